"""The kernels of csrc/nonlocal_channel.hip against the term-wise fp64 restatement of tests/channel_nl_cases.py, over its SWEEP table (every
16-channel tile count at its lowest and highest C, N = 1 ... 65 and ragged planes, more tiles than the chunk cap, signed features, per-sample
scales, tied extrema, the entry limits), and the join kernels against their fp64 definition.

mmif_nonlocal_channel_fwd / _bwd and mmif_fuse_join_fwd / _bwd are called through mmif._lib.lib on guarded buffers: every output sits inside a
larger allocation pre-filled with a sentinel, 64 guard floats on either side; each call gets a workspace of exactly the queried number of bytes of
1e30 garbage with a guard behind it.  After the calls: return codes 0, no sentinel left, nothing non-finite, guards untouched, inputs (and,
across the backward call, e, attn and the scalar block) bit-identical, and a second run on fresh buffers gives the same bits.

What is compared, element-wise within the derived rounding of the stored float32 word + tol * max |quantity| (norms: channel_nl_cases.err_*):
  E            against X X^T, and bitwise symmetric
  attn         against the row softmax
  lo, hi, r    lo, hi relative to hi - lo, r relative to itself (halved: it moves with both)
  positions    words 4-6 and 8-10 of the scalar block EQUAL the fp64 (b, i, j), first in C order of E[B, C, C]
  a = y - x    against A X            -- over the attention term, not over y, which x dominates
  d = dx - g   against tA + tB + tR   -- not over dx, which g dominates
tol = 8 x the float32 yardstick of the case and quantity (channel_nl_cases.tolerances: computed on the CPU from the inputs alone, nothing
measured on the code under test).  tests/test_channel_nl_oracle_cpu.py asserts that every mutant lies at least 20 tolerances away.

Tie cases hold the kernels to their OWN documented rule -- ties go to the smallest (sample, i C + j) -- which is not torch's even split.
"""
import ctypes

import numpy as np
import pytest
import torch

import channel_nl_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -7.5e28


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
    """forward, then backward on the forward kernels' own e, attn and scalar block, on fresh buffers"""

    def __init__(self, c):
        from mmif._lib import lib
        from mmif.tensor import stream_ptr
        x, g, _, _ = CC.reference(c.name)
        b, ch, h, w = c.shape
        self.x, self.g = Buf(x), Buf(g)
        self.y, self.e, self.attn, self.scal, self.dx = Buf(size=x.size), Buf(size=b * ch * ch), Buf(size=b * ch * ch), Buf(size=16), Buf(size=x.size)
        need = lib.mmif_nonlocal_channel_workspace(b, ch, h, w)
        self.ws = [Workspace(need), Workspace(need)]
        st = stream_ptr()
        rc = lib.mmif_nonlocal_channel_fwd(self.x.ptr, self.y.ptr, self.e.ptr, self.attn.ptr, self.scal.ptr, b, ch, h, w, self.ws[0].ptr, need, st)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc, lib.mmif_last_error())
        saved = [t.full.clone() for t in (self.e, self.attn, self.scal)]
        rc = lib.mmif_nonlocal_channel_bwd(self.x.ptr, self.e.ptr, self.attn.ptr, self.scal.ptr, self.g.ptr, self.dx.ptr, b, ch, h, w, self.ws[1].ptr,
                                           need, st)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc, lib.mmif_last_error())
        self.saved_unchanged = all(torch.equal(s.view(torch.int32), t.bits()) for s, t in zip(saved, (self.e, self.attn, self.scal)))
        self.outs = {"y": self.y, "e": self.e, "attn": self.attn, "scal": self.scal, "dx": self.dx}

    def same_bits(self, other):
        return all(torch.equal(t.bits(), other.outs[k].bits()) for k, t in self.outs.items())


@pytest.mark.parametrize("c", CC.SWEEP, ids=lambda c: c.name)
def test_kernels_equal_the_termwise_definition(c):
    x, g, ref, dist = CC.reference(c.name)
    tol = CC.tolerances(c.name)
    b, ch, h, w = c.shape
    run = Run(c)
    for name, t in run.outs.items():
        assert t.guards_untouched(), f"{c.name}: the guards around {name} were written"
        assert t.sentinels_left() == 0, f"{c.name}: {t.sentinels_left()} words of {name} still hold the sentinel"
    assert all(s.guard_untouched() for s in run.ws), f"{c.name}: the workspace was overrun"
    assert run.x.unchanged() and run.g.unchanged(), f"{c.name}: an input was written"
    assert run.saved_unchanged, f"{c.name}: the backward call wrote e, attn or the scalar block"
    y, dx = run.y.f32().reshape(c.shape), run.dx.f32().reshape(c.shape)
    e, attn = run.e.f32().reshape(b, ch, ch), run.attn.f32().reshape(b, ch, ch)
    scal = run.scal.f32()
    words = scal.view(np.int32)
    assert all(np.isfinite(v).all() for v in (y, dx, e, attn, scal[:3])), c.name
    assert not words[[3, 7, 11, 12, 13, 14, 15]].any(), (c.name, words)
    assert np.array_equal(e.view(np.int32), e.transpose(0, 2, 1).view(np.int32)), f"{c.name}: the stored energy is not symmetric bit for bit"

    pos_lo, pos_hi = tuple(int(k) for k in words[4:7]), tuple(int(k) for k in words[8:11])
    figs = {"e": CC.err_e(e, ref), "attn": CC.err_attn(attn, ref), "scalars": CC.err_scalars(scal[0], scal[1], scal[2], None, ref),
            "a": CC.err_a(y, x, ref), "d": CC.err_d(dx, g, ref)}
    near = {q: min((dist[k] for k in ms if k in dist), default=float("inf")) for q, ms in (("a", CC.MUTANTS_A), ("d", CC.MUTANTS_D))}
    print(f"{c.name} {c.shape} KC {c.kc}: " + "  ".join(f"{q} {figs[q]:.2e} (tol {tol[q]:.1e})" for q in CC.QUANTITIES)
          + f"  nearest mutants a {near['a']:.2e} d {near['d']:.2e}  argmin {pos_lo} argmax {pos_hi}")
    assert pos_lo == ref["pos_lo"] and pos_hi == ref["pos_hi"], (c.name, pos_lo, ref["pos_lo"], pos_hi, ref["pos_hi"])
    assert scal[0] == e[pos_lo] and scal[1] == e[pos_hi]
    for q in CC.QUANTITIES:
        assert figs[q] <= tol[q], (c.name, q, figs[q], tol[q])
    assert run.same_bits(Run(c)), f"{c.name}: a second forward + backward on fresh buffers differs"


def test_entry_limits():
    from mmif._lib import lib
    for n, c, h, w in ((1, 1, 4, 4), (0, 4, 4, 4), (65536, 4, 4, 4), (2, 257, 4, 4), (2, 4, 0, 4), (1, 4, 32768, 32768)):
        assert lib.mmif_nonlocal_channel_workspace(n, c, h, w) == 0, (n, c, h, w)
    need = lib.mmif_nonlocal_channel_workspace(1, 2, 1, 1)
    assert need > 0
    ws, bufs = Workspace(need), [Buf(size=16) for _ in range(5)]
    p = [t.ptr for t in bufs]
    assert lib.mmif_nonlocal_channel_fwd(p[0], p[1], p[2], p[3], p[4], 1, 1, 1, 1, ws.ptr, need, None) == -1          # n * c = 1
    assert lib.mmif_nonlocal_channel_fwd(p[0], p[1], p[2], p[3], p[4], 1, 2, 1, 1, ws.ptr, need - 4, None) == -3      # workspace too small
    assert lib.mmif_nonlocal_channel_bwd(p[0], p[1], p[2], p[3], p[4], p[0], 1, 257, 1, 1, ws.ptr, need, None) == -1
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in bufs)


# ------------------------------------------------------------------------------------------------------------------------------ the join
GRADS = ("dt1", "dt2", "ds1", "ds2", "dc1", "dc2")


class JoinRun:
    def __init__(self, mode, arrs):
        from mmif._lib import lib
        from mmif.tensor import stream_ptr
        sp, ch = mode != "ca", mode != "sa"
        have = (True, True, sp, sp, ch, ch)
        count = arrs[0].size
        self.ins = [Buf(a) if h else None for a, h in zip(arrs[:6], have)]
        self.g = Buf(arrs[6])
        self.out = Buf(size=count)
        self.grads = [Buf(size=count) if h else None for h in have]
        ptr = lambda t: t.ptr if t is not None else None
        st = stream_ptr()
        rc = lib.mmif_fuse_join_fwd(*(ptr(t) for t in self.ins), self.out.ptr, CC.JOIN_MODES[mode], count, st)
        assert rc == 0, (mode, count, rc, lib.mmif_last_error())
        rc = lib.mmif_fuse_join_bwd(*(ptr(t) for t in self.ins), self.g.ptr, *(ptr(t) for t in self.grads), CC.JOIN_MODES[mode], count, st)
        torch.cuda.synchronize()
        assert rc == 0, (mode, count, rc, lib.mmif_last_error())
        self.outs = [self.out] + [t for t in self.grads if t is not None]


@pytest.mark.parametrize("count", CC.JOIN_COUNTS)
@pytest.mark.parametrize("mode", CC.FUSION_MODES)
def test_join_equals_its_definition(mode, count):
    assert CC.JOIN_COUNTS[-1] > CC.JOIN_GRID_CAP * 256
    arrs = CC.join_inputs(count, 4500 + count % 97)
    sp, ch = mode != "ca", mode != "sa"
    ops = [a if h else None for a, h in zip(arrs[:6], (True, True, sp, sp, ch, ch))]
    ref_out, ref_grads = CC.join_def(mode, *ops, arrs[6], dt=np.float64)
    f32_out, f32_grads = CC.join_def(mode, *ops, arrs[6], dt=np.float32)
    run = JoinRun(mode, arrs)
    for t in run.outs:
        assert t.guards_untouched() and t.sentinels_left() == 0 and np.isfinite(t.f32()).all(), (mode, count)
    assert all(t.unchanged() for t in run.ins if t is not None) and run.g.unchanged()
    rows = [("out", run.out.f32(), ref_out, f32_out)] + [(n, t.f32(), r, f) for n, t, r, f in zip(GRADS, run.grads, ref_grads, f32_grads) if t is not None]
    assert [n for n, *_ in rows][1:] == [n for n, r in zip(GRADS, ref_grads) if r is not None]
    for name, got, ref, f32 in rows:
        (e_rest, e_own), (y_rest, y_own) = CC.join_err(got, ref, CC.PLANTED), CC.join_err(f32, ref, CC.PLANTED)
        print(f"join {mode} count {count} {name}: {e_rest:.2e} (tol {CC.TOL_FACTOR * y_rest:.1e})  planted, each relative to itself: {e_own:.2e} "
              f"(tol {CC.TOL_FACTOR * y_own:.1e})")
        assert e_rest <= CC.TOL_FACTOR * y_rest, (mode, count, name, e_rest, y_rest)
        assert e_own <= CC.TOL_FACTOR * y_own, (mode, count, name, "planted", e_own, y_own)
    again = JoinRun(mode, arrs)
    assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(run.outs, again.outs))


def test_join_refuses_maps_a_mode_does_not_use():
    from mmif._lib import lib
    bufs = [Buf(np.ones(8, np.float32)) for _ in range(7)]
    outs = [Buf(size=8) for _ in range(7)]
    p, o = [t.ptr for t in bufs], [t.ptr for t in outs]
    assert lib.mmif_fuse_join_fwd(p[0], p[1], p[2], p[3], p[4], p[5], o[0], 0, 8, None) == -1       # 'sa' with channel maps
    assert lib.mmif_fuse_join_fwd(p[0], p[1], None, None, p[4], p[5], o[0], 2, 8, None) == -1       # 'sca' without spatial maps
    assert lib.mmif_fuse_join_fwd(p[0], p[1], p[2], p[3], p[4], p[5], o[0], 4, 8, None) == -1       # no such mode
    assert lib.mmif_fuse_join_bwd(p[0], p[1], p[2], p[3], None, None, p[6], o[1], o[2], o[3], o[4], o[5], o[6], 0, 8, None) == -1
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in outs)
