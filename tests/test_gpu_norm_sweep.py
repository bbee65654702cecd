"""Every entry point of csrc/norm.hip (mmif_norm_act_fwd / _bwd, the staged cross-rank BatchNorm mmif_bn_moments / mmif_bn_apply_fwd /
mmif_bn_bwd_sums / mmif_bn_apply_bwd, mmif_act_fwd / _bwd) against its fp64 definition (tests/norm_cases.py), element-wise, with derived bounds.

Device buffers are built in torch straight from the stored arrays and the C ABI is called through mmif._lib.lib (mmif/tensor.py's wrappers
allocate their own outputs, which could not carry guards).  Every output sits inside a larger allocation pre-filled with the sentinel, 64
guard elements on either side, at an odd element offset in the cases marked so; the workspace is exactly mmif_norm_workspace() bytes of 1e30
garbage with a guard behind it.  After the call: every output element within its bound (selections bit-exact), guards and the workspace's
guard untouched, inputs bit-identical (the running buffers handed to kind 2, which ignores them, among them); a second call on fresh
buffers is bit-identical (the fixed-order claim of norm.hip's header comment).  Every got value must be finite: a NaN fails the comparison
and shows in the report.  An output passed as NULL cannot be watched: that the call returns and every other buffer's guards are intact is
all the evidence there is.  The staged cases are two emulated ranks (1 + 2 samples) with the fp64 vectors summed by a torch add on
the device between the calls.  Chained: the backward kernels on the forward kernels' own y and stats against the backward definition at
those arrays, and fused kind 0 against the staged calls without an all-reduce, bit for bit, at hw = 257, c = 257.
"""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import norm_cases as NC
from norm_cases import CASES, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
RATIOS = {}           # entry point, output -> [max err / bound, max err, checks]


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class Buf:
    """a device array of `size` elements inside a sentinel-filled allocation: GUARD (+ 1 when odd) elements in front, at least GUARD behind"""

    def __init__(self, values=None, size=None, dtype=torch.float32, odd=False):
        if values is not None:
            values = np.asarray(values, np.float64).reshape(-1)
            size = values.size
        self.size, self.off = size, GUARD + (1 if odd else 0)
        self.full = torch.full((size + 2 * GUARD + 2,), SENT, dtype=dtype, device=DEV)
        if values is not None and size:
            self.full[self.off:self.off + size] = torch.from_numpy(values).to(dtype).to(DEV)
        self.before = self.full.clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr() + self.off * self.full.element_size())

    @property
    def view(self):
        return self.full[self.off:self.off + self.size]

    def got(self):
        return self.view.cpu().numpy().astype(np.float64)

    def guards_untouched(self):
        g = torch.cat([self.full[:self.off], self.full[self.off + self.size:]])
        return bool((g == SENT).all())

    def unchanged(self):
        return torch.equal(_bits(self.full), _bits(self.before))


def _ptr(b):
    return None if b is None else b.ptr


class Workspace:
    """exactly `nbytes` (a multiple of 8) of 1e30 garbage, GUARD doubles of it behind"""

    def __init__(self, nbytes):
        assert nbytes % 8 == 0
        self.n = nbytes // 8
        self.full = torch.full((self.n + GUARD,), 1e30, dtype=torch.float64, device=DEV)
        self.ptr, self.nbytes = ctypes.c_void_p(self.full.data_ptr()), nbytes

    def guard_untouched(self):
        return bool((self.full[self.n:] == 1e30).all())


class Run:
    """the case's calls on fresh buffers: outs[name] = Buf per output of NC.define, ins = every operand that must come back bit-identical"""

    def __init__(self, c, o=None):
        from mmif._lib import check, lib
        from mmif.tensor import stream_ptr
        o = NC.operands(c) if o is None else o
        eps, mom, slope = c.scalars()
        st = stream_ptr()
        odd = c.offset
        self.outs, self.ins, self.ws = {}, [], []

        def inp(a, dtype=torch.float32):
            if a is None:
                return None
            b = Buf(a, dtype=dtype, odd=odd)
            self.ins.append(b)
            return b

        def out(name, size, present=True, dtype=torch.float32, init=None):
            """present = False: the output is passed as NULL"""
            if not present:
                return None
            b = Buf(init, size=size, dtype=dtype, odd=odd)
            self.outs[name] = b
            return b

        def ws():
            w = Workspace(lib.mmif_norm_workspace(c.n, c.c))
            self.ws.append(w)
            return w

        if c.ep == "act_fwd":
            x, y = inp(o["x"]), out("y", c.count)
            check(lib.mmif_act_fwd(x.ptr, y.ptr, c.count, c.act, slope, st), c.id)
        elif c.ep == "act_bwd":
            gy, y, dx = inp(o["gy"]), inp(o["y"]), out("dx", c.count)
            check(lib.mmif_act_bwd(gy.ptr, y.ptr, dx.ptr, c.count, c.act, slope, st), c.id)
        elif c.ep == "norm_fwd":
            x, gamma, beta = inp(o["x"]), inp(o["gamma"]), inp(o["beta"])
            y, stats = out("y", o["x"].size), out("stats", 2 * (c.n if c.kind == 2 else 1) * c.c)
            rm = rv = None
            if c.kind == 1 or NC.gn_given_running(c):          # inputs: eval reads them, kind 2 ignores them
                rm, rv = inp(o["running"][0]), inp(o["running"][1])
            elif c.kind == 0 and c.running:
                rm, rv = out("running_mean", c.c, init=o["running"][0]), out("running_var", c.c, init=o["running"][1])
            w = ws()
            check(lib.mmif_norm_act_fwd(x.ptr, _ptr(gamma), _ptr(beta), y.ptr, stats.ptr, _ptr(rm), _ptr(rv), c.n, c.c, c.hw, c.kind, eps, mom, c.act,
                                        slope, w.ptr, w.nbytes, st), c.id)
        elif c.ep == "norm_bwd":
            x, y, gy, gamma = inp(o["x"]), inp(o["y"]), inp(o["gy"]), inp(o["gamma"])
            stats = inp(NC.stats_array(o["mean"], o["rstd"]))
            dx, dg, db = out("dx", o["x"].size), out("dgamma", c.c, c.dgamma), out("dbeta", c.c, c.dbeta)
            w = ws()
            check(lib.mmif_norm_act_bwd(x.ptr, y.ptr, gy.ptr, stats.ptr, _ptr(gamma), dx.ptr, _ptr(dg), _ptr(db), c.n, c.c, c.hw, c.kind, c.act, slope,
                                        w.ptr, w.nbytes, st), c.id)
        else:
            self._staged(c, o, lib, check, st, inp, out, eps, mom, slope)
        torch.cuda.synchronize()

    def _staged(self, c, o, lib, check, st, inp, out, eps, mom, slope):
        """two ranks: the statistics stage on each part, the fp64 vectors added on the device (the all-reduce), the apply stage on each part"""
        ranks = list(NC._rank_slices())
        xs = [inp(o["x"][sl]) for _, sl in ranks]
        gamma = inp(o["gamma"])
        moments = []
        for (r, sl), x in zip(ranks, xs):
            n_r = sl.stop - sl.start
            if c.ep == "staged_fwd":
                chan = out(f"chan_sums_r{r}", 2 * c.c + 1, dtype=torch.float64)
            else:          # the backward cases need the count too; their forward sums are not an output under test
                chan = Buf(size=2 * c.c + 1, dtype=torch.float64, odd=c.offset)
            w = Workspace(lib.mmif_norm_workspace(n_r, c.c))
            self.ws.append(w)
            check(lib.mmif_bn_moments(x.ptr, chan.ptr, n_r, c.c, c.hw, w.ptr, w.nbytes, st), c.id)
            moments.append(chan)
        total = moments[0].view + moments[1].view                     # the SUM all-reduce, count included
        total_before = total.clone()
        tptr = ctypes.c_void_p(total.data_ptr())
        if c.ep == "staged_fwd":
            beta = inp(o["beta"])
            for (r, sl), x in zip(ranks, xs):
                n_r = sl.stop - sl.start
                y, stats = out(f"y_r{r}", o["x"][sl].size), out(f"stats_r{r}", 2 * c.c)
                rm = out(f"running_mean_r{r}", c.c, c.running, init=o["running"][0] if c.running else None)
                rv = out(f"running_var_r{r}", c.c, c.running, init=o["running"][1] if c.running else None)
                check(lib.mmif_bn_apply_fwd(x.ptr, tptr, _ptr(gamma), _ptr(beta), y.ptr, stats.ptr, _ptr(rm), _ptr(rv), n_r, c.c, c.hw, eps, mom, c.act,
                                            slope, st), c.id)
        else:
            stats = inp(NC.stats_array(o["mean"], o["rstd"]))
            ys, gys, sums = [inp(o["y"][sl]) for _, sl in ranks], [inp(o["gy"][sl]) for _, sl in ranks], []
            for (r, sl), x, y, gy in zip(ranks, xs, ys, gys):
                n_r = sl.stop - sl.start
                bs = out(f"chan_sums_r{r}", 2 * c.c, dtype=torch.float64)
                dg, db = out(f"dgamma_r{r}", c.c, c.dgamma), out(f"dbeta_r{r}", c.c, c.dbeta)
                w = Workspace(lib.mmif_norm_workspace(n_r, c.c))
                self.ws.append(w)
                check(lib.mmif_bn_bwd_sums(x.ptr, y.ptr, gy.ptr, stats.ptr, bs.ptr, _ptr(dg), _ptr(db), n_r, c.c, c.hw, c.act, slope, w.ptr, w.nbytes, st), c.id)
                sums.append(bs)
            bsum = sums[0].view + sums[1].view
            bsum_before = bsum.clone()
            count = ctypes.c_void_p(total.data_ptr() + 2 * c.c * 8)          # the summed count, on the device
            for (r, sl), x, y, gy in zip(ranks, xs, ys, gys):
                n_r = sl.stop - sl.start
                dx = out(f"dx_r{r}", o["x"][sl].size)
                check(lib.mmif_bn_apply_bwd(x.ptr, y.ptr, gy.ptr, stats.ptr, _ptr(gamma), ctypes.c_void_p(bsum.data_ptr()), count, dx.ptr, n_r, c.c, c.hw,
                                            c.act, slope, st), c.id)
            torch.cuda.synchronize()
            assert torch.equal(bsum, bsum_before), f"{c.id}: the reduced backward sums were written"
        torch.cuda.synchronize()
        assert torch.equal(total, total_before), f"{c.id}: the reduced moments were written"
        assert float(total[2 * c.c]) == c.n * c.hw

    def same_bits(self, other):
        return all(torch.equal(_bits(b.full), _bits(other.outs[k].full)) for k, b in self.outs.items())


def _check(c, o, got):
    want, bound = np.asarray(o.want, np.float64).reshape(-1), np.broadcast_to(np.asarray(o.bound, np.float64), o.want.shape).reshape(-1)
    assert got.shape == want.shape, (c.id, o.name, got.shape, want.shape)
    if not want.size:
        return
    left = got == SENT
    assert not left.any(), f"{c.id} {o.name}: {int(left.sum())} elements still hold the sentinel, first at {int(np.argmax(left))}"
    nonfinite = ~np.isfinite(got)          # every want of this family is finite
    err = np.where(nonfinite, np.inf, np.abs(np.where(nonfinite, 0.0, got) - want))
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    if o.exact:          # a selection: the float32 bits themselves, so that -0.0 is not +0.0
        differ = got.astype(np.float32).view(np.int32) != want.astype(np.float32).view(np.int32)
        ratio = np.where(differ & (ratio == 0), np.inf, ratio)
    r = float(ratio.max())
    name = o.name.split("_r")[0] if c.ep.startswith("staged") else o.name
    e = RATIOS.setdefault(f"{c.ep} {name}", [0.0, 0.0, 0])
    e[0], e[1], e[2] = max(e[0], min(r, 1e30)), max(e[1], float(err.max())), e[2] + 1
    print(f"{c.id} {o.name}: max err {err.max():.3e}, max err / bound {r:.3f}")
    bad = ~(err <= bound) | ~(ratio < np.inf)          # (a NaN or inf in got, or a wrong bit of a selection, is bad)
    if bad.any():
        i = int(np.argmax(ratio))
        idx = tuple(int(k) for k in np.unravel_index(i, o.want.shape))
        raise AssertionError(f"{c.id} {o.name}: {int(bad.sum())} of {bad.size} elements beyond the bound{' (bit-exact)' if o.exact else ''}; worst at "
                             f"{idx}: got {got[i]!r}, want {want[i]!r}, err {err[i]:.3e}, bound {bound[i]:.3e} (err / bound {r:.3g})")


def _sweep(c, o=None):
    run = Run(c, o)
    outs = NC.define(c, o=o)
    assert {d.name for d in outs} == set(run.outs), (sorted(d.name for d in outs), sorted(run.outs))
    for name, b in run.outs.items():
        assert b.guards_untouched(), f"{c.id}: the guards around {name} were written"
    assert all(w.guard_untouched() for w in run.ws), f"{c.id}: the workspace was overrun"
    assert all(b.unchanged() for b in run.ins), f"{c.id}: an input was written"
    for d in outs:
        _check(c, d, run.outs[d.name].got())
    return run


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_kernel_equals_definition(c):
    run = _sweep(c)
    assert run.same_bits(Run(c)), f"{c.id}: a second call on fresh buffers differs"


CHAINED = [c for c in CASES if c.ep == "norm_fwd" and c.gamma and c.beta and not c.plant and c.m > 1][:15:2] + \
    [c for c in CASES if c.ep == "staged_fwd" and c.gamma][:2]


@pytest.mark.parametrize("c", CHAINED, ids=lambda c: c.id)
def test_backward_kernel_on_the_forward_kernels_own_output(c):
    """forward kernel -> backward kernel on the kernel's own y and stats, against the backward definition evaluated at those same arrays"""
    o = NC.operands(c)
    f = Run(c)
    staged = c.ep == "staged_fwd"
    y = np.concatenate([f.outs[f"y_r{r}"].got() for r, _ in NC._rank_slices()]) if staged else f.outs["y"].got()
    stats = (f.outs["stats_r0"] if staged else f.outs["stats"]).got().reshape(-1, 2)
    if staged:
        assert torch.equal(_bits(f.outs["stats_r0"].view), _bits(f.outs["stats_r1"].view)), "both ranks hold the same statistics"
    shape = (c.n, c.c, 1, 1) if c.kind == 2 else (1, c.c, 1, 1)
    gy = NC.f32(np.random.default_rng(c.hw * 7 + c.c).standard_normal(c.shape))
    ob = dict(x=o["x"], gamma=o["gamma"], beta=o["beta"], y=y.reshape(c.shape), gy=gy, mean=stats[:, 0].reshape(shape), rstd=stats[:, 1].reshape(shape))
    _sweep(dataclasses.replace(c, ep="staged_bwd" if staged else "norm_bwd"), ob)


def test_fused_batchnorm_equals_the_staged_calls_past_one_block():
    """kind 0 of mmif_norm_act_fwd / _bwd against mmif_bn_moments -> mmif_bn_apply_fwd and mmif_bn_bwd_sums -> mmif_bn_apply_bwd without an
    all-reduce, bit for bit, at hw = 257 (a second trip of the moment loops, ragged) and c = 257 (a second block of the finish kernels)"""
    from mmif._lib import check, lib
    from mmif.tensor import stream_ptr
    n, c, hw, act, slope, eps, mom = 3, 257, 257, 2, 0.2, 1e-5, 0.1
    rng = np.random.default_rng(257)
    st = stream_ptr()
    x, gy = Buf(rng.standard_normal(n * c * hw) * 1.5 + 0.3), Buf(rng.standard_normal(n * c * hw))
    gamma, beta = Buf(1 + 0.3 * rng.standard_normal(c)), Buf(0.3 * rng.standard_normal(c))
    rm0, rv0 = rng.standard_normal(c), rng.uniform(0.5, 2, c)
    need = lib.mmif_norm_workspace(n, c)
    res = []
    for staged in (False, True):
        y, stats, dx, dg, db = Buf(size=n * c * hw), Buf(size=2 * c), Buf(size=n * c * hw), Buf(size=c), Buf(size=c)
        rm, rv = Buf(rm0), Buf(rv0)
        w = Workspace(need)
        if staged:
            chan, bs = Buf(size=2 * c + 1, dtype=torch.float64), Buf(size=2 * c, dtype=torch.float64)
            check(lib.mmif_bn_moments(x.ptr, chan.ptr, n, c, hw, w.ptr, w.nbytes, st))
            check(lib.mmif_bn_apply_fwd(x.ptr, chan.ptr, gamma.ptr, beta.ptr, y.ptr, stats.ptr, rm.ptr, rv.ptr, n, c, hw, eps, mom, act, slope, st))
            check(lib.mmif_bn_bwd_sums(x.ptr, y.ptr, gy.ptr, stats.ptr, bs.ptr, dg.ptr, db.ptr, n, c, hw, act, slope, w.ptr, w.nbytes, st))
            count = ctypes.c_void_p(chan.ptr.value + 2 * c * 8)
            check(lib.mmif_bn_apply_bwd(x.ptr, y.ptr, gy.ptr, stats.ptr, gamma.ptr, bs.ptr, count, dx.ptr, n, c, hw, act, slope, st))
        else:
            check(lib.mmif_norm_act_fwd(x.ptr, gamma.ptr, beta.ptr, y.ptr, stats.ptr, rm.ptr, rv.ptr, n, c, hw, 0, eps, mom, act, slope, w.ptr, w.nbytes, st))
            check(lib.mmif_norm_act_bwd(x.ptr, y.ptr, gy.ptr, stats.ptr, gamma.ptr, dx.ptr, dg.ptr, db.ptr, n, c, hw, 0, act, slope, w.ptr, w.nbytes, st))
        torch.cuda.synchronize()
        assert w.guard_untouched()
        res.append((y, stats, rm, rv, dx, dg, db))
    for name, a, b in zip(("y", "stats", "running_mean", "running_var", "dx", "dgamma", "dbeta"), *res):
        assert a.guards_untouched() and b.guards_untouched(), name
        assert not bool((a.view == SENT).any()), name
        assert torch.equal(_bits(a.full), _bits(b.full)), f"{name}: staged differs from fused"


def test_platform_tanh_accuracy_is_what_the_bound_assumes():
    """the figure TANH_ULP rests on: torch.tanh in float32 on the device against float64 tanh, in ulp of the float32 result, over [-12, 12]"""
    z = torch.linspace(-12.0, 12.0, 1 << 22, dtype=torch.float32, device=DEV)
    got = torch.tanh(z).cpu().numpy().astype(np.float64)
    want = np.tanh(z.cpu().numpy().astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(got - want) / ulp).max())
    print(f"device tanh (float32): max error {worst:.3f} ulp over [-12, 12]; TANH_ULP_MEASURED = {NC.TANH_ULP_MEASURED}")
    RATIOS["platform tanh ulp"] = [worst, 0.0, 1]
    assert worst <= NC.TANH_ULP_MEASURED


def test_zz_report_error_over_bound_per_entry_point():
    """prints the measured maximum of every entry point and output as a fraction of its bound ($MMIF_NORM_SWEEP_REPORT: also as JSON)"""
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f"{k:28s} max err/bound {r:8.4f}   max err {e:.3e}   checks {n}")
    path = os.environ.get("MMIF_NORM_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
