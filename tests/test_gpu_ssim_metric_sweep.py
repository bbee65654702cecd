"""mmif_metric_ssim_maps / mmif_metric_msssim_any (csrc/metric_ssim.hip) and the calc_ssim / calc_msssim / fusion_metrics routes of
core/metric.py against the float64 definition of tests/ssim_metric_cases.py, over its whole case table: every window 1..11 with and
without padding, windows shrunk to the image, map extents around the 16-pixel tile, the pyramid from 9 x 9 up, batches 1..3, data ranges
1 and 255, blends, near-flat, anti-correlated and constant images.

The C entry points are called through mmif._lib.lib: every output sits between 64 sentinel words in a larger allocation, the workspace is
exactly the queried number of bytes with a guard behind it.  After each call: return code 0, no sentinel left, nothing non-finite, guards and
inputs untouched.  Maps are compared element-wise and means absolutely, each within SC.reference(case)['tol'] -- 8 x the error of the float32
CPU evaluation of the same case, floored at 2^-22 max(|ref|, 0.1); nothing measured on the kernels.  tests/test_ssim_metric_oracle_cpu.py
shows every wrong-but-plausible variant to lie at least 20 of these tolerances away.

Largest errors measured on an MI355X (absolute; the kernels compute in fp64, so what is left is the float32 rounding of the stored maps
and the summation order of the means):
  maps   2.98e-8 = 2^-25, half a float32 ulp below 1 (at most 0.125 of the tolerance, where only its floor applies)
  means  7.1e-14 for the per-sample ssim / cs means, 6.7e-13 for the level means, 1.2e-13 for the MS-SSIM values (all on near-flat
         cases: under 1e-9 of their tolerances); mmif_metric_msssim_any against the float32 mmif_metric_msssim at 161 x 176: 5.0e-5
"""
import ctypes

import numpy as np
import pytest
import torch

import ssim_metric_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -7.5e28


class Buf:
    """`size` elements of `dtype` inside a sentinel-filled allocation with GUARD elements on either side"""

    def __init__(self, size, dtype=torch.float32, values=None):
        self.size, self.item = size, torch.empty((), dtype=dtype).element_size()
        self.full = torch.full((size + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        if values is not None:
            self.full[GUARD:GUARD + size] = torch.from_numpy(np.array(values)).reshape(-1).to(DEV)
        self.before = self.full.clone()
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + GUARD * self.item)

    def get(self):
        return self.full[GUARD:GUARD + self.size].cpu().numpy()

    def check_written(self, what):
        assert bool((self.full[:GUARD] == SENT).all()) and bool((self.full[GUARD + self.size:] == SENT).all()), f"{what}: guard words were written"
        v = self.full[GUARD:GUARD + self.size]
        assert int((v == SENT).sum()) == 0, f"{what}: sentinel left"
        assert bool(torch.isfinite(v).all()), f"{what}: non-finite value"

    def check_unchanged(self, what):
        assert torch.equal(self.full, self.before), f"{what}: was written"


class Workspace:
    """exactly `nbytes` of garbage with GUARD bytes behind"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.full = torch.full((nbytes + GUARD,), 0x7f, dtype=torch.uint8, device=DEV)
        self.ptr = ctypes.c_void_p(self.full.data_ptr())

    def check(self, what):
        assert bool((self.full[self.nbytes:] == 0x7f).all()), f"{what}: the workspace was overrun"


def _lib():
    from mmif._lib import lib
    from mmif.tensor import stream_ptr
    return lib, stream_ptr()


def run_maps(a, b, win, pad, dr, want=(True, True, True)):
    """mmif_metric_ssim_maps on numpy [n,1,h,w] -> (ssim map | None, cs map | None, sums [n,2] | None)"""
    lib, st = _lib()
    n, _, h, w = a.shape
    k = min(win, h, w)
    p = k // 2 if pad else 0
    hm, wm = h + 2 * p - k + 1, w + 2 * p - k + 1
    ia, ib = Buf(a.size, values=a), Buf(b.size, values=b)
    sm = Buf(n * hm * wm) if want[0] else None
    cm = Buf(n * hm * wm) if want[1] else None
    su = Buf(2 * n, torch.float64) if want[2] else None
    need = lib.mmif_metric_ssim_maps_workspace(n, h, w, win, pad)
    assert need > 0
    ws = Workspace(need) if want[2] else None
    rc = lib.mmif_metric_ssim_maps(ia.ptr, ib.ptr, n, h, w, win, pad, dr, sm.ptr if sm else None, cm.ptr if cm else None, su.ptr if su else None,
                                   ws.ptr if ws else None, need if ws else 0, st)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.mmif_last_error())
    ia.check_unchanged("img1")
    ib.check_unchanged("img2")
    for t, what in ((sm, "ssim map"), (cm, "cs map"), (su, "sums")):
        if t is not None:
            t.check_written(what)
    if ws:
        ws.check("ssim_maps")
    shp = (n, 1, hm, wm)
    return (sm.get().reshape(shp) if sm else None, cm.get().reshape(shp) if cm else None, su.get().reshape(n, 2) if su else None)


def run_ms(a, b, f, win, pad, dr):
    """mmif_metric_msssim_any -> [2, 6, n] float64"""
    lib, st = _lib()
    n, _, h, w = a.shape
    ia, i_f = Buf(a.size, values=a), Buf(f.size, values=f)
    ib = Buf(b.size, values=b) if b is not None else None
    out = Buf(12 * n, torch.float64)
    need = lib.mmif_metric_msssim_any_workspace(n, h, w)
    assert need > 0
    ws = Workspace(need)
    rc = lib.mmif_metric_msssim_any(ia.ptr, ib.ptr if ib else None, i_f.ptr, n, h, w, win, pad, dr, out.ptr, ws.ptr, need, st)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.mmif_last_error())
    for t in (ia, ib, i_f):
        if t is not None:
            t.check_unchanged("input")
    out.check_written("msssim out")
    ws.check("msssim_any")
    return out.get().reshape(2, 6, n)


def _err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


@pytest.mark.parametrize("name", SC.SSIM_CASES)
def test_ssim_maps_against_definition(name):
    _, h, w, n, win, pad, dist = SC.CASES[name]
    a, b = SC.build(name)
    ref = SC.reference(name)
    sm, cm, su = run_maps(a, b, win, pad, SC.data_range(dist))
    assert sm.shape == ref["ssim"].shape, (sm.shape, ref["ssim"].shape)
    cnt = sm.shape[-2] * sm.shape[-1]
    errs = {"ssim": _err(sm, ref["ssim"]), "cs": _err(cm, ref["cs"]), "ssim_mean": _err(su[:, 0] / cnt, ref["ssim_mean"]),
            "cs_mean": _err(su[:, 1] / cnt, ref["cs_mean"])}
    print(name, " ".join(f"{k} {e:.2e} (tol {ref['tol'][k]:.1e}, float32 CPU {ref['err32'][k]:.1e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= ref["tol"][k], (name, k, e, ref["tol"][k])
    if dist == 'const' and win == 1:
        assert (sm == 1.0).all()
    # each output alone gives the same bits
    s2, _, _ = run_maps(a, b, win, pad, SC.data_range(dist), (True, False, False))
    _, c2, _ = run_maps(a, b, win, pad, SC.data_range(dist), (False, True, False))
    _, _, u2 = run_maps(a, b, win, pad, SC.data_range(dist), (False, False, True))
    assert np.array_equal(s2, sm) and np.array_equal(c2, cm) and np.array_equal(u2, su), name


@pytest.mark.parametrize("name", SC.MS_CASES)
def test_msssim_any_against_definition(name):
    _, h, w, n, win, pad, dist = SC.CASES[name]
    a, b = SC.build(name)
    ref = SC.reference(name)
    dr = SC.data_range(dist)
    out = run_ms(a, None, b, win, pad, dr)
    assert np.array_equal(out[1], out[0]), "b == NULL: pair 2 repeats pair 1"
    two = run_ms(a, a, b, win, pad, dr)
    assert np.array_equal(two[0], out[0]) and np.array_equal(two[1], out[0]), "two equal pairs give the bits of one"
    val = SC.ms_value(torch.from_numpy(out[0])).numpy()
    pooled = float(SC.ms_value(torch.from_numpy(out[0]).mean(dim=1)))
    errs = {"levels": _err(out[0], ref["levels"]), "value": _err(val, ref["value"]), "pooled": abs(pooled - float(ref["pooled"]))}
    print(name, " ".join(f"{k} {e:.2e} (tol {ref['tol'][k]:.1e}, float32 CPU {ref['err32'][k]:.1e})" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= ref["tol"][k], (name, k, e, ref["tol"][k])
    if dist == 'anti':
        assert (out[0, :4] < 0).any(), "the anti-correlated pair must drive a level cs mean below the 1e-7 clamp"
    if min(h, w) >= 161 and not pad and win == 11:
        # the 11-tap pyramid kernel (mmif_metric_msssim, float32) computes the same six rows: the existing suite holds it to 1e-4
        lib, st = _lib()
        ta, tf = (torch.from_numpy(np.array(x)).to(DEV) for x in (a, b))
        old = torch.empty((2, 6, n), dtype=torch.float32, device=DEV)
        nb = lib.mmif_metric_msssim_workspace(n, h, w)
        wsp = torch.empty(nb, dtype=torch.uint8, device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lib.mmif_metric_msssim(p(ta), None, p(tf), n, h, w, dr, p(old), p(wsp), nb, st) == 0
        d = _err(old[0].double().cpu().numpy(), out[0])
        print(name, f"against mmif_metric_msssim: {d:.2e}")
        assert d <= 1e-4


def test_sample_values_do_not_depend_on_the_batch():
    """a B = 3 call and its three B = 1 calls agree bitwise on the per-sample sums and on every MS-SSIM row"""
    for name in ("ssim-20x23-b3-k3-valid-anti", "ssim-15x33-b3-k11-pad-rand255", "ssim-26x26-b3-k11-valid-blend"):
        _, h, w, n, win, pad, dist = SC.CASES[name]
        assert n == 3
        a, b = SC.build(name)
        _, _, su = run_maps(a, b, win, pad, SC.data_range(dist), (False, False, True))
        for i in range(3):
            _, _, one = run_maps(a[i:i + 1], b[i:i + 1], win, pad, SC.data_range(dist), (False, False, True))
            assert np.array_equal(one[0], su[i]), (name, i)
    for name in ("ms-9x300-b3-k11-valid-anti", "ms-40x40-b3-k8-pad-flat"):
        _, h, w, n, win, pad, dist = SC.CASES[name]
        assert n == 3
        a, b = SC.build(name)
        out = run_ms(a, None, b, win, pad, SC.data_range(dist))
        for i in range(3):
            one = run_ms(a[i:i + 1], None, b[i:i + 1], win, pad, SC.data_range(dist))
            assert np.array_equal(one[:, :, 0], out[:, :, i]), (name, i)


@pytest.fixture
def no_stock(monkeypatch):
    """every function of core/_stock.py raises"""
    import types

    from core import _stock

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"core._stock.{name} was called")
        return f
    for k, v in list(vars(_stock).items()):
        if isinstance(v, types.FunctionType) and v.__module__ == _stock.__name__:
            monkeypatch.setattr(_stock, k, refuse(k))
    return _stock


def test_python_routes_never_touch_stock(no_stock):
    """the whole case table through calc_ssim (scalars and maps) and calc_msssim, and fusion_metrics at 64 x 80, B = 8"""
    import core.metric as M
    with pytest.raises(AssertionError, match="_stock"):
        M.calc_ssim(torch.zeros(1, 1, 12, 12), torch.zeros(1, 1, 12, 12), 7)       # the guard works: CPU tensors still go to stock
    for name in SC.SSIM_CASES:
        _, h, w, n, win, pad, dist = SC.CASES[name]
        a, b = (torch.from_numpy(np.array(x)).to(DEV) for x in SC.build(name))
        ref, dr = SC.reference(name), SC.data_range(dist)
        s, c = M.calc_ssim(a, b, win, dr, bool(pad), True, True)
        assert s.dtype == torch.float32 and s.dim() == 0 and c.dtype == torch.float32 and c.dim() == 0
        # (returned in float32, as the stock composition's were: half a float32 ulp, a quarter of the tolerance's floor)
        assert abs(float(s) - float(ref["ssim_pooled"])) <= ref["tol"]["ssim_pooled"] and abs(float(c) - float(ref["cs_pooled"])) <= ref["tol"]["cs_pooled"], name
        sm, cm = M.calc_ssim(a, b, win, dr, bool(pad), False, True)
        assert sm.dtype == torch.float32 and tuple(sm.shape) == ref["ssim"].shape and tuple(cm.shape) == ref["cs"].shape
        assert _err(sm.cpu().numpy(), ref["ssim"]) <= ref["tol"]["ssim"] and _err(cm.cpu().numpy(), ref["cs"]) <= ref["tol"]["cs"], name
        only = M.calc_ssim(a, b, win, dr, bool(pad), False, False)
        assert torch.equal(only, sm), name
    for name in SC.MS_CASES:
        _, h, w, n, win, pad, dist = SC.CASES[name]
        a, b = (torch.from_numpy(np.array(x)).to(DEV) for x in SC.build(name))
        ref = SC.reference(name)
        v = M.calc_msssim(a, b, win, SC.data_range(dist), bool(pad))
        assert v.dtype == torch.float64 and v.dim() == 0
        tol = ref["tol"]["pooled"]
        if min(h, w) >= M.MSSSIM_MIN and win == 11 and not pad:
            tol = max(tol, 1e-4 * abs(float(ref["pooled"])))      # this call keeps mmif_metric_msssim (float32), held to 1e-4 by its own tests
        assert abs(float(v) - float(ref["pooled"])) <= tol, (name, float(v), float(ref["pooled"]), tol)
    # uint8, float64 and non-contiguous inputs go through the same conversion
    a8 = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (2, 1, 20, 46)).astype(np.uint8)).to(DEV)
    x, y = a8[..., ::2], a8[..., 1::2]
    want = M.calc_ssim(x.float().contiguous(), y.float().contiguous(), 8, 255.0, True, False, True)
    for got in (M.calc_ssim(x, y, 8, 255.0, True, False, True), M.calc_ssim(x.double(), y.double(), 8, 255.0, True, False, True)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # fusion_metrics below 161 px: ssim and msssim of every sample from one mmif_metric_msssim_any call
    rng = np.random.RandomState(11)
    a = (255.0 * rng.rand(8, 1, 64, 80)).astype(np.float32)
    b = (255.0 * rng.rand(8, 1, 64, 80)).astype(np.float32)
    f = np.clip(0.5 * (a + b) + 4.0 * rng.randn(8, 1, 64, 80), 0, 255).astype(np.float32)
    r = M.fusion_metrics(*(torch.from_numpy(t).to(DEV) for t in (a, b, f)))
    lv = {dt: (SC.ms_levels(a, f, 11, False, 255.0, dt), SC.ms_levels(b, f, 11, False, 255.0, dt)) for dt in (torch.float64, torch.float32)}
    ssim = {dt: ((p[0][5] + p[1][5]) * 0.5).double().numpy() for dt, p in lv.items()}
    ms = {dt: ((SC.ms_value(p[0]) + SC.ms_value(p[1])) * 0.5).double().numpy() for dt, p in lv.items()}
    for key, d in (("ssim", ssim), ("msssim", ms)):
        tol = SC.tol_of(d[torch.float64], d[torch.float32])
        e = _err(r[key].cpu().numpy(), d[torch.float64])
        print(f"fusion_metrics 8x64x80 {key}: {e:.2e} (tol {tol:.1e})")
        assert r[key].dtype == torch.float64 and tuple(r[key].shape) == (8,) and e <= tol, (key, e, tol)
