"""The kernels of csrc/attn_fuse.hip against the float64 definition of tests/attn_fuse_cases.py, through the C ABI, over its case table:
n = 1 ... 3, c = 1 ... 257, planes from 1 x 1 to 300 x 300 (widths and a base pointer that break 16-byte alignment, ragged tiles, several
blocks per channel sum, more work items than either grid cap), planted ties, all-zero pixel vectors and planes, pools below, on and above the
clamp, signed features with negative sums; every one of the 5 x 2 x 4 + SEDRFuse combinations on the small shapes.

mmif_attn_fuse_fwd / _bwd are called through mmif._lib.lib on guarded buffers: every array sits inside a larger allocation pre-filled with a
sentinel, 64 guard floats on either side; each call gets a workspace of exactly the queried number of bytes of 1e30 garbage with a guard behind
it (backward gets a fresh one: it may need nothing forward left).  After the calls: return codes 0, no sentinel left, nothing non-finite, guards
untouched, inputs (and, across the backward call, the pools) bit-identical, and a second run on fresh buffers gives the same bits.

Every term -- the pools s1, s2, c1, c2 in their own right, out, dt1, dt2 -- is compared element-wise in the norm of attn_fuse_cases.err against
tol = 8 x the float32 numpy evaluation's error of that case, combination and term (computed on the CPU from the inputs alone); the positions of
the channel maxima must EQUAL the definition's (first in row-major order).  tests/test_attn_fuse_oracle_cpu.py shows every mutant at least 20
tolerances away.
"""
import ctypes

import numpy as np
import pytest
import torch

import attn_fuse_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -7.5e28


class Buf:
    """a device array of `size` 4-byte words inside a sentinel-filled allocation with GUARD words on either side (+ `offset` words in front, which
    takes the array off 16-byte alignment)"""

    def __init__(self, values=None, size=None, offset=0):
        if values is not None:
            values = np.array(values, np.float32).reshape(-1)          # (a copy: the shared reference arrays are read-only)
            size = values.size
        self.size, self.lo = size, GUARD + offset
        self.full = torch.full((size + 2 * GUARD + offset,), SENT, dtype=torch.float32, device=DEV)
        if values is not None:
            self.full[self.lo:self.lo + size] = torch.from_numpy(values).to(DEV)
        self.before = self.full.clone()
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + self.lo * 4)

    def bits(self):
        return self.full.view(torch.int32)

    def f32(self):
        return self.full[self.lo:self.lo + self.size].cpu().numpy()

    def i32(self):
        return self.bits()[self.lo:self.lo + self.size].cpu().numpy()

    def guards_untouched(self):
        return bool((self.full[:self.lo] == SENT).all()) and bool((self.full[self.lo + self.size:] == SENT).all())

    def sentinels_left(self):
        return int((self.bits()[self.lo:self.lo + self.size] == self.before.view(torch.int32)[0]).sum())

    def unchanged(self):
        return torch.equal(self.bits(), self.before.view(torch.int32))


class Workspace:
    """exactly `nbytes` of 1e30 garbage, GUARD floats of it behind"""

    def __init__(self, nbytes, offset=0):
        assert nbytes > 0 and nbytes % 4 == 0
        self.n, self.nbytes = nbytes // 4, nbytes
        self.full = torch.full((self.n + GUARD + offset,), 1e30, dtype=torch.float32, device=DEV)
        self.ptr = ctypes.c_void_p(self.full.data_ptr() + offset * 4)
        self.end = offset + self.n

    def guard_untouched(self):
        return bool((self.full[self.end:] == 1e30).all())


POOLS = ("s1", "s2", "c1", "c2", "ci1", "ci2")


class Run:
    """forward, then backward on the forward kernels' own pools, on fresh buffers"""

    def __init__(self, arrs, combo, offset=0):
        from mmif._lib import lib
        from mmif.tensor import stream_ptr
        t1, t2, g = arrs
        n, c, h, w = t1.shape
        mode, sm, cm = combo
        codes = (AC.MODE_CODE[mode], AC.SPATIAL_CODE[sm], AC.CHANNEL_CODE[cm])
        sp, ch = AC.uses(mode)
        mx = ch and cm == "max"
        self.ins = [Buf(t1, offset=offset), Buf(t2, offset=offset), Buf(g, offset=offset)]
        new = lambda use, size: Buf(size=size, offset=offset) if use else None
        self.pools = dict(zip(POOLS, (new(sp, n * h * w), new(sp, n * h * w), new(ch, n * c), new(ch, n * c), new(mx, n * c), new(mx, n * c))))
        self.out, self.d1, self.d2 = (Buf(size=t1.size, offset=offset) for _ in range(3))
        need = lib.mmif_attn_fuse_workspace(n, c, h, w, *codes)
        self.ws = [Workspace(need, offset), Workspace(need, offset)]
        ptr = lambda t: t.ptr if t is not None else None
        pp = [ptr(self.pools[k]) for k in POOLS]
        st = stream_ptr()
        rc = lib.mmif_attn_fuse_fwd(self.ins[0].ptr, self.ins[1].ptr, self.out.ptr, *pp, n, c, h, w, *codes, self.ws[0].ptr, need, st)
        torch.cuda.synchronize()
        assert rc == 0, (combo, rc, lib.mmif_last_error())
        saved = {k: t.full.clone() for k, t in self.pools.items() if t is not None}
        rc = lib.mmif_attn_fuse_bwd(self.ins[0].ptr, self.ins[1].ptr, *pp, self.ins[2].ptr, self.d1.ptr, self.d2.ptr, n, c, h, w, *codes,
                                    self.ws[1].ptr, need, st)
        torch.cuda.synchronize()
        assert rc == 0, (combo, rc, lib.mmif_last_error())
        self.pools_unchanged = all(torch.equal(s.view(torch.int32), self.pools[k].bits()) for k, s in saved.items())
        self.outs = {"out": self.out, "d1": self.d1, "d2": self.d2, **{k: t for k, t in self.pools.items() if t is not None}}

    def same_bits(self, other):
        return all(torch.equal(t.bits(), other.outs[k].bits()) for k, t in self.outs.items())

    def terms(self, shape):
        n, c, h, w = shape
        o = dict.fromkeys(AC.TERMS + ("ci1", "ci2"))
        for k, t in self.outs.items():
            o[k] = t.i32().reshape(n, c) if k in ("ci1", "ci2") else t.f32().reshape(shape if k in ("out", "d1", "d2") else (n, -1))
        return o


@pytest.mark.parametrize("c", AC.CASES, ids=lambda c: c.name)
def test_kernels_equal_the_definition(c):
    arrs = AC.inputs(c.name)
    worst = {}
    for combo in AC.combos(c):
        ref, tol = AC.reference(c.name, combo)
        run = Run(arrs, combo, c.offset)
        tag = f"{c.name} {combo}"
        for name, t in run.outs.items():
            assert t.guards_untouched(), f"{tag}: the guards around {name} were written"
            assert t.sentinels_left() == 0, f"{tag}: {t.sentinels_left()} words of {name} still hold the sentinel"
        assert all(s.guard_untouched() for s in run.ws), f"{tag}: the workspace was overrun"
        assert all(t.unchanged() for t in run.ins), f"{tag}: an input was written"
        assert run.pools_unchanged, f"{tag}: the backward call wrote a pool"
        got = run.terms(c.shape)
        for k in ("ci1", "ci2"):
            assert (ref[k] is None) == (got[k] is None), (tag, k)
            if ref[k] is not None:
                assert np.array_equal(got[k], ref[k]), (tag, k, got[k], ref[k])
        figs = AC.errors(got, ref)
        print(f"{tag}: " + "  ".join(f"{k} {figs[k]:.2e} (tol {tol[k]:.1e})" for k in figs))
        for k, v in figs.items():
            assert v <= tol[k], (tag, k, v, tol[k])
            worst[k] = max(worst.get(k, 0.0), v / tol[k])
        assert run.same_bits(Run(arrs, combo, c.offset)), f"{tag}: a second forward + backward on fresh buffers differs"
    print(f"{c.name}: worst error in tolerances " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", ["n3c16_5x13", "n3c2_33x37"])
def test_a_sample_does_not_depend_on_its_batch(name):
    """sample 1 of the batch of 3 is bit-identical to the same sample alone: pools, positions, out and both gradients"""
    t1, t2, g = AC.inputs(name)
    shape = t1.shape
    for combo in AC.COMBOS:
        batch = Run((t1, t2, g), combo).terms(shape)
        alone = Run((t1[1:2], t2[1:2], g[1:2]), combo).terms((1,) + shape[1:])
        for k, v in alone.items():
            if v is not None:
                assert np.array_equal(v.view(np.int32), np.ascontiguousarray(batch[k][1:2]).view(np.int32)), (name, combo, k)


def test_entry_limits_and_refusals():
    from mmif._lib import lib
    for bad in ((0, 4, 4, 4, 3, 2, 0), (65536, 4, 4, 4, 3, 2, 0), (2, 0, 4, 4, 3, 2, 0), (2, 65536, 4, 4, 3, 2, 0), (2, 4, 0, 4, 3, 2, 0),
                (1, 4, 32768, 32768, 3, 2, 0), (2, 4, 4, 4, 4, 2, 0), (2, 4, 4, 4, 3, 6, 0), (2, 4, 4, 4, 3, 2, 2)):
        assert lib.mmif_attn_fuse_workspace(*bad) == 0, bad
    dims = (2, 4, 4, 4)
    need = lib.mmif_attn_fuse_workspace(*dims, 3, 4, 1)
    assert need > 0
    ws, bufs = Workspace(need), [Buf(np.ones(128, np.float32)) for _ in range(12)]
    p = [t.ptr for t in bufs]
    all6 = p[3:9]
    fwd = lambda pools, dims, codes, nbytes=need: lib.mmif_attn_fuse_fwd(p[0], p[1], p[2], *pools, *dims, *codes, ws.ptr, nbytes, None)
    assert fwd(all6, dims, (4, 4, 1)) == -1                                   # no such mode
    assert fwd(all6, dims, (3, 6, 1)) == -1 and fwd(all6, dims, (3, 4, 2)) == -1
    assert fwd(all6, dims, (0, 4, 1)) == -1                                   # 'sa' given channel pools
    assert fwd(p[3:5] + [None] * 4, dims, (1, 4, 1)) == -1                    # 'ca' given spatial pools
    assert fwd([None, None] + p[5:9], dims, (2, 4, 1)) == -1                  # 'sca' without spatial pools
    assert fwd(all6, dims, (3, 4, 0)) == -1                                   # positions given to 'avg'
    assert fwd(p[3:7] + [None, None], dims, (3, 4, 1)) == -1                  # 'max' without positions
    assert fwd(all6, (2, 0, 4, 4), (3, 4, 1)) == -1                           # c = 0
    assert fwd(all6, dims, (3, 4, 1), need - 4) == -3                         # a short workspace
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], *all6, None, p[10], p[11], *dims, 3, 4, 1, ws.ptr, need, None) == -1
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], *all6, p[9], p[10], p[11], *dims, 3, 4, 1, ws.ptr, need - 4, None) == -3
    assert lib.mmif_attn_fuse_bwd(p[0], p[1], None, None, *p[5:9], p[9], p[10], p[11], *dims, 3, 4, 1, ws.ptr, need, None) == -1
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in bufs) and ws.guard_untouched() and bool((ws.full == 1e30).all())
