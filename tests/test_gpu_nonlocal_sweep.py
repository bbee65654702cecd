"""The ten kernels of csrc/nonlocal.hip against the term-wise fp64 restatement of tests/nonlocal_cases.py, over the SWEEP table: every channel
width KC at its lowest and highest C, one key, one pair, ragged multi-pair key loops, signed features, per-sample scales, tied extrema.

mmif_nonlocal_spatial_fwd / _bwd are called through mmif._lib.lib (mmif/tensor.py's wrappers allocate exact-size outputs, which could not carry
guards).  y, l, the 16-word scalar block and dx each sit inside a larger allocation pre-filled with a sentinel, 64 guard floats on either side;
each call gets a workspace of exactly the queried number of bytes of 1e30 garbage with a guard behind it.  After the calls: return codes 0, no
sentinel left, nothing non-finite, guards untouched, x and g (and, across the backward call, y, l and the scalar block) bit-identical.

What is compared (norms and tolerances: tests/nonlocal_cases.py, 8 x the error of the float32 numpy evaluation of the same formulas, nothing
measured on the code under test):
  a = y - x      against S P            max |.| / max |a|   -- over the attention term, not over y, which x dominates
  l              against sum exp(Z)     max |.| / max |l|
  lo, hi, r      against fp64           lo, hi relative to hi - lo, r relative to itself
  positions      words 4-6 and 8-10 of the scalar block as int32 EQUAL the fp64 (b, i, j), first in C order of E[B, N, M]; j a real key index
  d = dx - g     against tB + tC + tD + tR, element-wise  |.| <= 2^-23 |dx_ref| + tol max |d|   -- not over dx, which g dominates
Each case prints its error beside the distance of the nearest mutant (softmax -> 1 / M; one gradient term dropped; the routed terms sent to the
runners-up); tests/test_nonlocal_oracle_cpu.py asserts that every mutant lies at least 20 tolerances away, so passing here excludes them all.

Tie cases hold the kernels to their OWN documented rule -- ties go to the smallest (sample, position) -- which is not torch's: the composition's
amin / amax backward splits the gradient evenly among tied elements.  For the duplicated-sample case the "runners-up" mutant is exactly
"routed to sample 1 instead of sample 0".
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import nonlocal_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -7.5e28
FIGS = {}          # case -> dict of measured errors and nearest-mutant distances


class Buf:
    """a device array of `size` floats inside a sentinel-filled allocation with GUARD floats on either side"""

    def __init__(self, values=None, size=None):
        if values is not None:
            values = np.array(values, np.float32).reshape(-1)          # (a copy: the shared reference arrays are read-only)
            size = values.size
        self.size = size
        self.full = torch.full((size + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        if values is not None:
            self.full[GUARD:GUARD + size] = torch.from_numpy(values).to(DEV)
        self.before = self.full.clone()
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + GUARD * 4)

    def bits(self):
        return self.full.view(torch.int32)

    def f32(self):
        return self.full[GUARD:GUARD + self.size].cpu().numpy()

    def guards_untouched(self):
        return bool((self.full[:GUARD] == SENT).all()) and bool((self.full[GUARD + self.size:] == SENT).all())

    def sentinels_left(self):
        return int((self.bits()[GUARD:GUARD + self.size] == self.before.view(torch.int32)[0]).sum())

    def unchanged(self):
        return torch.equal(self.bits(), self.before.view(torch.int32))


class Workspace:
    """exactly `nbytes` of 1e30 garbage, GUARD floats of it behind"""

    def __init__(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        self.n, self.nbytes = nbytes // 4, nbytes
        self.full = torch.full((self.n + GUARD,), 1e30, dtype=torch.float32, device=DEV)
        self.ptr = ctypes.c_void_p(self.full.data_ptr())

    def guard_untouched(self):
        return bool((self.full[self.n:] == 1e30).all())


class Run:
    """forward, then backward on the forward kernels' own y, l and scalar block, on fresh buffers"""

    def __init__(self, c):
        from mmif._lib import lib
        from mmif.tensor import stream_ptr
        x, g, _, _ = NC.reference(c.name)
        b, ch, h, w = c.shape
        self.x, self.g = Buf(x), Buf(g)
        self.y, self.l, self.scal, self.dx = Buf(size=x.size), Buf(size=b * h * w), Buf(size=16), Buf(size=x.size)
        need = lib.mmif_nonlocal_spatial_workspace(b, ch, h, w)
        self.ws = [Workspace(need), Workspace(need)]
        st = stream_ptr()
        self.rc_fwd = lib.mmif_nonlocal_spatial_fwd(self.x.ptr, self.y.ptr, self.l.ptr, self.scal.ptr, b, ch, h, w, self.ws[0].ptr, need, st)
        torch.cuda.synchronize()
        assert self.rc_fwd == 0, (c.name, self.rc_fwd, lib.mmif_last_error())
        saved = [t.full.clone() for t in (self.y, self.l, self.scal)]
        self.rc_bwd = lib.mmif_nonlocal_spatial_bwd(self.x.ptr, self.y.ptr, self.l.ptr, self.scal.ptr, self.g.ptr, self.dx.ptr, b, ch, h, w,
                                                    self.ws[1].ptr, need, st)
        torch.cuda.synchronize()
        assert self.rc_bwd == 0, (c.name, self.rc_bwd, lib.mmif_last_error())
        self.saved_unchanged = all(torch.equal(s.view(torch.int32), t.bits()) for s, t in zip(saved, (self.y, self.l, self.scal)))
        self.outs = {"y": self.y, "l": self.l, "scal": self.scal, "dx": self.dx}

    def same_bits(self, other):
        return all(torch.equal(t.bits(), other.outs[k].bits()) for k, t in self.outs.items())


def _sweep(c):
    x, g, ref, dist = NC.reference(c.name)
    b, ch, h, w = c.shape
    m = (h // 8) * (w // 8)
    run = Run(c)
    for name, t in run.outs.items():
        assert t.guards_untouched(), f"{c.name}: the guards around {name} were written"
        assert t.sentinels_left() == 0, f"{c.name}: {t.sentinels_left()} words of {name} still hold the sentinel"
    assert all(s.guard_untouched() for s in run.ws), f"{c.name}: the workspace was overrun"
    assert run.x.unchanged() and run.g.unchanged(), f"{c.name}: an input was written"
    assert run.saved_unchanged, f"{c.name}: the backward call wrote y, l or the scalar block"
    y, l, dx = run.y.f32().reshape(c.shape), run.l.f32().reshape(b, h * w), run.dx.f32().reshape(c.shape)
    scal = run.scal.f32()
    words = scal.view(np.int32)
    assert np.isfinite(y).all() and np.isfinite(l).all() and np.isfinite(dx).all() and np.isfinite(scal[:3]).all(), c.name
    assert not words[[3, 7, 11, 12, 13, 14, 15]].any(), (c.name, words)

    pos_lo, pos_hi = tuple(int(k) for k in words[4:7]), tuple(int(k) for k in words[8:11])
    e_a = NC.err_max(y.astype(np.float64) - x, ref["a"])
    e_l = NC.err_max(l, ref["l"])
    e_s = NC.err_scalars(scal[0], scal[1], scal[2], ref)
    e_d = NC.err_d(dx.astype(np.float64) - g, ref, g)
    near_a = min((dist[k] for k in NC.MUTANTS_A if k in dist), default=float("inf"))
    near_d = min((dist[k], k) for k in NC.MUTANTS_D if k in dist)
    FIGS[c.name] = dict(a=e_a, l=e_l, scalars=e_s, d=e_d, tol=list(c.tol), nearest_a=near_a, nearest_d=near_d[0], nearest_d_mutant=near_d[1])
    print(f"{c.name} {c.shape} KC {c.kc} JT {c.jt}: a {e_a:.2e} (tol {c.tol[0]:.1e}, uniform-softmax mutant at {near_a:.2e})  l {e_l:.2e} (tol {c.tol[1]:.1e})  "
          f"lo/hi/r {e_s:.2e} (tol {c.tol[3]:.1e})  d {e_d:.2e} (tol {c.tol[2]:.1e}, nearest mutant {near_d[1]} at {near_d[0]:.2e})  "
          f"argmin {pos_lo} argmax {pos_hi}")
    assert pos_lo == ref["pos_lo"] and pos_hi == ref["pos_hi"], (c.name, pos_lo, ref["pos_lo"], pos_hi, ref["pos_hi"])
    assert 0 <= pos_lo[2] < m and 0 <= pos_hi[2] < m
    assert e_s <= c.tol[3], (c.name, "lo/hi/r", e_s, scal[:3], ref["lo"], ref["hi"], ref["r"])
    assert e_l <= c.tol[1], (c.name, "l", e_l)
    assert e_a <= c.tol[0], (c.name, "a", e_a)
    assert e_d <= c.tol[2], (c.name, "d", e_d)
    return run


@pytest.mark.parametrize("c", NC.SWEEP, ids=lambda c: c.name)
def test_kernels_equal_the_termwise_definition(c):
    run = _sweep(c)
    assert run.same_bits(Run(c)), f"{c.name}: a second forward + backward on fresh buffers differs"


@pytest.mark.parametrize("c", [c for c in NC.SWEEP if c.tie], ids=lambda c: c.name)
def test_ties_go_to_the_smallest_sample_and_position(c):
    """the kernels' rule, not torch's even split.  _sweep has compared a and d with the first-position reference; here the positions themselves"""
    scal = Run(c).scal.f32()
    words = scal.view(np.int32)
    pos_lo, pos_hi = tuple(int(k) for k in words[4:7]), tuple(int(k) for k in words[8:11])
    if c.tie == "zero":
        assert pos_lo == (0, NC.ZERO_PIXEL, 0), pos_lo          # an M-way (B M-way) tie of exact zeros: sample 0, key 0 of that pixel
        assert scal[0] == 0.0
    else:
        _, _, ref, dist = NC.reference(c.name)
        assert pos_lo == ref["pos_lo"] and pos_hi == ref["pos_hi"] and pos_lo[0] == 0 and pos_hi[0] == 0
        assert dist["second"] >= 20 * c.tol[2]                     # routing to sample 1 instead is far outside what _sweep accepts


def test_zz_report():
    """prints every case's measured errors ($MMIF_NONLOCAL_SWEEP_REPORT: also as JSON)"""
    for k, f in FIGS.items():
        print(f"{k:20s} a {f['a']:.2e} / {f['tol'][0]:.1e}   l {f['l']:.2e} / {f['tol'][1]:.1e}   d {f['d']:.2e} / {f['tol'][2]:.1e}   lo/hi/r {f['scalars']:.2e} / "
              f"{f['tol'][3]:.1e}   nearest mutants: a {f['nearest_a']:.2e}, d {f['nearest_d']:.2e} ({f['nearest_d_mutant']})")
    path = os.environ.get("MMIF_NONLOCAL_SWEEP_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump(FIGS, fh, indent=1, sort_keys=True)
