"""mmif_clip_adam_step (csrc/misc.hip: sumsq_kernel + adam_kernel) against its fp64 definition (tests/optim_cases.py), element-wise, with
derived bounds: buffers up to three times the 1024-block cap, every clip regime, grad_scale, bias-correction step, zero and non-finite
gradients.

Device buffers are built in torch straight from the stored arrays and the C ABI is called through mmif._lib.lib.  params, both moments and
norm_out sit inside larger allocations pre-filled with the sentinel, 64 guard floats on either side, at an odd float offset in the cases
marked so; the workspace is exactly mmif_clip_adam_workspace() bytes of 1e30 garbage with a guard behind it.  After the call: every element
within its bound (NaN and inf exactly where the definition has them; an untouched parameter bit-identical), guards untouched, the gradients
bit-identical, a NULL norm_out not written; a second call on fresh buffers is bit-identical (adam_kernel's fixed-order claim).  Chained: three
consecutive steps on device state, each against the definition evaluated on the state the device held before it, and the whole against
the definition's float64 trajectory within the one-step bounds carried forward.
"""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import optim_cases as OC
from optim_cases import CASES, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
RATIOS = {}


def _bits(t):
    return t.view(torch.int32)


class Buf:
    def __init__(self, values=None, size=None, odd=False):
        if values is not None:
            values = np.asarray(values, np.float64).reshape(-1)
            size = values.size
        self.size, self.off = size, GUARD + (1 if odd else 0)
        self.full = torch.full((size + 2 * GUARD + 2,), SENT, dtype=torch.float32, device=DEV)
        if values is not None:
            self.full[self.off:self.off + size] = torch.from_numpy(values).to(torch.float32).to(DEV)
        self.before = self.full.clone()
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + 4 * self.off)

    def got(self):
        return self.full[self.off:self.off + self.size].cpu().numpy().astype(np.float64)

    def guards_untouched(self):
        return bool((torch.cat([self.full[:self.off], self.full[self.off + self.size:]]) == SENT).all())

    def unchanged(self):
        return torch.equal(_bits(self.full), _bits(self.before))


class State:
    """device state of one flat parameter buffer; step() is one mmif_clip_adam_step on it"""

    def __init__(self, c, o):
        from mmif._lib import lib
        self.c = c
        self.p, self.m, self.v = (Buf(o[k], odd=c.offset) for k in ("p", "m", "v"))
        self.norm = Buf(size=1, odd=c.offset)
        nbytes = lib.mmif_clip_adam_workspace(c.numel)
        assert nbytes % 4 == 0
        self.ws_n = nbytes // 4
        self.ws = torch.full((self.ws_n + GUARD,), 1e30, dtype=torch.float32, device=DEV)
        self.nbytes = nbytes

    def step(self, g, step):
        from mmif._lib import check, lib
        from mmif.tensor import stream_ptr
        c = self.c
        self.ws[:self.ws_n] = 1e30          # nothing may be taken from the workspace uncomputed
        gb = Buf(g, odd=c.offset)
        check(lib.mmif_clip_adam_step(self.p.ptr, gb.ptr, self.m.ptr, self.v.ptr, c.numel, OC.LR, OC.B1, OC.B2, OC.ADAM_EPS, step, c.max_norm,
                                      c.grad_scale, self.norm.ptr if c.norm_out else None, ctypes.c_void_p(self.ws.data_ptr()), self.nbytes,
                                      stream_ptr()), c.id)
        torch.cuda.synchronize()
        assert gb.unchanged(), f"{c.id}: the gradients were written"
        assert bool((self.ws[self.ws_n:] == 1e30).all()), f"{c.id}: the workspace was overrun"
        for name, b in (("params", self.p), ("exp_avg", self.m), ("exp_avg_sq", self.v), ("norm_out", self.norm)):
            assert b.guards_untouched(), f"{c.id}: the guards around {name} were written"
        if not c.norm_out:
            assert self.norm.unchanged(), f"{c.id}: a NULL norm_out was written"

    def outs(self):
        return {"params": self.p, "exp_avg": self.m, "exp_avg_sq": self.v, "norm_out": self.norm}

    def same_bits(self, other):
        return all(torch.equal(_bits(a.full), _bits(b.full)) for a, b in zip(self.outs().values(), other.outs().values()))


def _check(c, d, got, what=""):
    want, bound = d.want.reshape(-1), d.bound.reshape(-1)
    assert got.shape == want.shape
    nan_ok = np.array_equal(np.isnan(got), np.isnan(want))
    assert nan_ok, (f"{c.id}{what} {d.name}: NaN in {int(np.isnan(got).sum())} elements, the definition has {int(np.isnan(want).sum())} "
                    f"(first difference at {int(np.argmax(np.isnan(got) != np.isnan(want)))})")
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{c.id}{what} {d.name}: infinities differ"
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    r = float(ratio.max())
    e = RATIOS.setdefault(f"clip_adam_step {d.name}", [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], min(r, 1e30)), max(e[1], float(err.max())), e[2] + 1
    print(f"{c.id}{what} {d.name}: max err {err.max():.3e}, max err / bound {r:.3f}")
    bad = err > bound
    if bad.any():
        i = int(np.argmax(ratio))
        raise AssertionError(f"{c.id}{what} {d.name}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst at [{i}]: got {got[i]!r}, "
                             f"want {want[i]!r}, err {err[i]:.3e}, bound {bound[i]:.3e} (err / bound {r:.3g})")


def _run(c):
    o = OC.operands(c)
    s = State(c, o)
    s.step(o["g"], c.step)
    return s


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_kernel_equals_definition(c):
    s = _run(c)
    for d in OC.define(c):
        _check(c, d, s.outs()[d.name].got())
    if c.special in ("zero", "stretch"):          # the unused-parameter contract of mmif/optim.py: bit-identical, not merely within a bound
        sl = slice(None) if c.special == "zero" else OC.stretch(c)
        lo, hi = s.p.off + (sl.start or 0), s.p.off + (c.numel if sl.stop is None else sl.stop)
        assert torch.equal(_bits(s.p.full[lo:hi]), _bits(s.p.before[lo:hi])), f"{c.id}: a parameter with zero gradient and zero moments moved"
    assert s.same_bits(_run(c)), f"{c.id}: a second call on fresh buffers differs"


@pytest.mark.parametrize("c", [c for c in CASES if not c.special and c.numel in (257, 262145) and c.clip in ("above", "tiny", "below")],
                         ids=lambda c: c.id)
def test_three_consecutive_steps_on_device_state(c):
    """steps c.step, +1, +2 on the state the device itself carries, fresh gradients each time.  Every step is held to the definition (and its
    one-step bounds) evaluated on the fp32 state the device held before it, and the device's state to the definition's own float64
    trajectory from the case's start, within the one-step bounds carried forward (optim_cases.propagate)"""
    o = OC.operands(c)
    s = State(c, o)
    rng = np.random.default_rng(c.numel + c.step)
    st = {k: o[k] for k in ("p", "m", "v")}          # what the device held before the step
    tr, E = dict(st), None                           # the definition's trajectory and the bounds carried along it
    for k in range(3):
        g = o["g"] if k == 0 else OC.f32(o["g"] * rng.uniform(0.9, 1.1, c.numel))
        s.step(g, c.step + k)
        ck = dataclasses.replace(c, step=c.step + k)
        for d in OC.define_on(ck, dict(g=g, **st)):
            _check(c, d, s.outs()[d.name].got(), f" step+{k}")
        ot = dict(g=g, **tr)
        r = OC.adam_on(tr["p"], g, tr["m"], tr["v"], ck.step, c.max_norm, c.grad_scale)
        E = OC.propagate(E, r, OC.bounds(ck, ot, r))
        for name, key in (("params", "p"), ("exp_avg", "m"), ("exp_avg_sq", "v")):
            _check(c, OC.Out(name + " (trajectory)", r[key], E[key]), s.outs()[name].got(), f" step+{k}")
        tr = dict(p=r["p"], m=r["m"], v=r["v"])
        st = dict(p=s.p.got(), m=s.m.got(), v=s.v.got())


def test_zz_report_error_over_bound_per_output():
    """prints the measured maximum of every output as a fraction of its bound ($MMIF_OPTIM_SWEEP_REPORT: also as JSON)"""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:28s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_OPTIM_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
