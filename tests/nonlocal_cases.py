"""Cases and a numpy float64 restatement of spatial_pooling(x, 'nl') (reference core/fusion.py:96-113) for golden F21.

The fixture tests/golden/f21_nonlocal.npz (written by tests/golden/make_golden_nonlocal.py from the reference's own code in float64)
holds results only; the inputs are rebuilt here from seeds.  Features are non-negative, like post-ReLU feature maps, and float32-exact,
so that the fp32 kernels and the float64 oracles start from the same numbers.  The gradient is that of sum(y * upstream(case)).

Arrays of more than SAMPLE_ABOVE elements are stored as a flat strided sample (sample_index) to keep the fixture small; the restatement
below is checked against those samples on the CPU and then serves as the full-tensor float64 reference of the GPU tests.

The second half is the table of tests/test_gpu_nonlocal_sweep.py: SWEEP, a term-wise float64 restatement (nonlocal_terms_f64, whose pieces sum
to nonlocal_f64), the same formulas in float32 (nonlocal_terms_f32: the yardstick of the sweep's tolerances) and the mutants, wrong-but-plausible
references that the kernels' error must stay far away from.
"""
import dataclasses
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F21 = os.path.join(HERE, "golden", "f21_nonlocal.npz")

# name -> (shape, seed, per-sample scale)
CASES = {
    "c112": ((2, 112, 24, 40), 2101, None),
    "ragged": ((1, 20, 27, 45), 2102, None),      # 27 x 45: rows 24.. and columns 40.. are queries that feed no key
    "m1": ((1, 16, 8, 8), 2103, None),            # M = 1: S == 1, dZ == 0
    "b3c7": ((3, 7, 16, 16), 2104, None),
    "scale2": ((2, 12, 16, 24), 2105, (1.0, 3.0)),  # sample 1 three times sample 0's scale: the global min / max couples them
}
TIE_GAP = 1e-6       # the two smallest and the two largest energies differ by more than this fraction of hi - lo
SAMPLE_ABOVE = 6000


def inputs(name):
    """x (float32, non-negative) of a case"""
    shape, seed, scale = CASES[name]
    rng = np.random.default_rng(seed)
    x = (rng.random(shape) ** 2).astype(np.float32)
    if scale is not None:
        x *= np.asarray(scale, np.float32).reshape(-1, 1, 1, 1)
    return x


def upstream(name):
    """dL/dy of a case (float32, both signs)"""
    shape, seed, _ = CASES[name]
    return np.random.default_rng(seed + 5000).standard_normal(shape).astype(np.float32)


def big_inputs(shape=(2, 112, 128, 128), seed=2199):
    """the 2 x 112 x 128 x 128 case of the GPU test: x and dL/dy"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) ** 2).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def sample_index(size):
    """flat indices a stored array holds: all of them up to SAMPLE_ABOVE elements, else every k-th with k odd (so that the sample walks
    through all channels, rows and columns)"""
    if size <= SAMPLE_ABOVE:
        return np.arange(size)
    k = -(-size // SAMPLE_ABOVE) | 1
    return np.arange(0, size, k)


def pool8(x):
    b, c, h, w = x.shape
    ph, pw = h // 8, w // 8
    return x[:, :, :ph * 8, :pw * 8].reshape(b, c, ph, 8, pw, 8).mean(axis=(3, 5))


def nonlocal_f64(x, g=None):
    """float64 restatement with the explicit backward formulas.  Returns dict(y, dx (if g), lo, hi, gap_lo, gap_hi): the gaps are the
    distances between the two smallest / two largest energies as fractions of hi - lo (the tie guard)."""
    x = np.asarray(x, np.float64)
    b, c, h, w = x.shape
    ph, pw = h // 8, w // 8
    n, m = h * w, ph * pw
    xq = x.reshape(b, c, n).transpose(0, 2, 1)             # [B, N, C]
    p = pool8(x).reshape(b, c, m).transpose(0, 2, 1)       # [B, M, C]
    e = xq @ p.transpose(0, 2, 1)                          # [B, N, M]
    flat = e.reshape(-1)
    lo2 = np.partition(flat, 1)[:2] if flat.size > 1 else np.array([flat[0], np.inf])
    hi2 = -np.partition(-flat, 1)[:2] if flat.size > 1 else np.array([flat[0], -np.inf])
    lo, hi = lo2.min(), hi2.max()
    r = 1.0 / (hi - lo)
    z = (e - lo) * r
    pe = np.exp(z)
    s = pe / pe.sum(axis=2, keepdims=True)
    y = s @ p + xq
    out = {"y": y.transpose(0, 2, 1).reshape(b, c, h, w), "lo": lo, "hi": hi,
           "gap_lo": (lo2.max() - lo2.min()) * r, "gap_hi": (hi2.max() - hi2.min()) * r}
    if g is None:
        return out
    gq = np.asarray(g, np.float64).reshape(b, c, n).transpose(0, 2, 1)
    d = (gq * (y - xq)).sum(axis=2, keepdims=True)         # D_i = g_i . (y_i - x_i)
    ds = gq @ p.transpose(0, 2, 1)                         # dS = g P^T
    dz = s * (ds - d)                                      # dZ = S o (dS - D)
    t = (dz * z).sum()                                     # T = sum dZ o Z
    dxq = gq + r * (dz @ p)                                # dx = g + r dZ P
    dp = s.transpose(0, 2, 1) @ gq + r * (dz.transpose(0, 2, 1) @ xq)   # dP = S^T g + r dZ^T x
    # through the two global scalars: the rows of dZ sum to 0, so d_lo = r T at the argmin of E, d_hi = -r T at the argmax
    for pos, dv in ((np.unravel_index(np.argmin(e), e.shape), r * t), (np.unravel_index(np.argmax(e), e.shape), -r * t)):
        bb, i, j = pos
        dxq[bb, i] += dv * p[bb, j]
        dp[bb, j] += dv * xq[bb, i]
    dx = dxq.transpose(0, 2, 1).reshape(b, c, h, w).copy()
    # dx += avgpool^T(dP): each dP row / 64 over its 8 x 8 block
    dpi = dp.transpose(0, 2, 1).reshape(b, c, ph, pw) / 64.0
    dx[:, :, :ph * 8, :pw * 8] += np.repeat(np.repeat(dpi, 8, axis=2), 8, axis=3)
    out["dx"] = dx
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the sweep
# Every product of csrc/nonlocal.hip term by term.  With E = x^T P over all of (B, N, M), Z = (E - lo) r, S = softmax_M(Z):
#   a  = S P                     the attention term y - x
#   l  = sum_j exp(Z)            the saved row sums
#   tB = r dZ P                  dZ = S o (g P^T - D),  D_i = g_i . (y_i - x_i)
#   tC = pool8^T(S^T g) / 64
#   tD = pool8^T(r dZ^T x) / 64
#   tR                           the two terms through lo and hi: d_lo = r T at the argmin element of E, d_hi = -r T at the argmax, T = sum dZ o Z,
#                                each into dx of its query (times P_j) and, through pool8^T, into the 8 x 8 block of its key (times x_i / 64)
# and dx = g + tB + tC + tD + tR.  Ties: the kernels route to the first position in (sample, query, key) order, which is np.argmin / np.argmax on
# E[B, N, M] in C order.  That is the kernels' own documented rule, NOT torch's, whose amin / amax backward splits the
# gradient evenly among tied elements: the tie cases below hold the kernels to their rule and say nothing about the composition.


def kc_for(c):
    """mirror of kc_for in csrc/nonlocal.hip: the 16-channel tiles the kernels run for C channels"""
    need = (c + 15) // 16
    return next(k for k in (1, 2, 4, 7, 8, 12, 16) if k >= need)


def jt_for(h, w):
    """mirror of NlGeo::JT: 16-key tiles, rounded up to whole 32-key pairs"""
    return ((h // 8) * (w // 8) + 31) // 32 * 2


@dataclasses.dataclass(frozen=True)
class Sweep:
    """tol = (a, l, d, lo/hi/r): 8 x the figures of float32_errors(name), the error of nonlocal_terms_f32 against nonlocal_terms_f64 in the norms
    of err_max / err_d / err_energy, rounded up to two significant digits (both evaluated on the CPU; test_nonlocal_oracle_cpu.py holds the live
    figure to a quarter of each constant).  The factor 8: the kernels sum in another order than numpy (4-wide matrix steps, 16-key tiles, split
    query chunks) and use expf, not a correctly rounded exp.  kc and jt are what the case claims to exercise, checked against kc_for / jt_for."""
    name: str
    shape: tuple
    seed: int
    signed: bool
    kc: int
    jt: int
    tol: tuple
    scale: tuple = None
    tie: str = None       # "zero": every channel of query pixel ZERO_PIXEL of every sample is 0;  "dup": every sample is a bit-copy of sample 0


ZERO_PIXEL = 77           # row 3, column 5 of the 16 x 24 tie cases

SWEEP = [
    Sweep("c1_m1", (1, 1, 8, 8), 3301, False, 1, 2, (1.3e-06, 9.8e-07, 1.5e-05, 3.7e-07)),               # N = 64: less than one block
    Sweep("c16", (1, 16, 16, 16), 3102, False, 1, 2, (2.4e-06, 1.3e-06, 9.1e-06, 1.5e-06)),
    Sweep("c17_m17", (2, 17, 8, 136), 3103, False, 2, 2, (3.4e-06, 9.2e-07, 4e-05, 1.7e-06)),          # a full key tile plus one key
    Sweep("c32_m34", (1, 32, 16, 136), 3104, True, 2, 4, (3.3e-05, 1.5e-06, 1.5e-05, 1.2e-06)),          # second pair with 30 padded keys
    Sweep("c33_m32", (1, 33, 32, 64), 3305, False, 4, 2, (3.7e-06, 1.1e-06, 3.3e-05, 3.2e-06)),          # exactly one pair
    Sweep("c64_ragged", (2, 64, 33, 65), 3106, True, 4, 2, (2.2e-05, 1.3e-06, 5.8e-06, 1.5e-06)),        # a row and a column that feed no key; N = 2145 = 16 * 134 + 1
    Sweep("c65_m35", (1, 65, 40, 56), 3107, False, 7, 4, (4.4e-06, 3.3e-06, 1.8e-05, 5.7e-06)),          # two padded channel tiles
    Sweep("c96_m9", (1, 96, 24, 24), 3108, True, 7, 2, (1.3e-05, 1.2e-06, 1.3e-05, 1.4e-06)),            # one padded channel tile
    Sweep("c112", (2, 112, 16, 24), 3109, False, 7, 2, (3e-06, 3.1e-06, 4.2e-05, 8e-06)),
    Sweep("c113_m36", (1, 113, 32, 72), 3110, True, 8, 4, (3e-05, 1.6e-06, 1.9e-05, 1.7e-06)),
    Sweep("c128_m34", (1, 128, 16, 136), 3111, False, 8, 4, (4.2e-06, 1.2e-06, 2e-05, 9.1e-06)),
    Sweep("c129", (1, 129, 16, 16), 3112, True, 12, 2, (5.7e-06, 1.1e-06, 5.1e-06, 3.8e-07)),
    Sweep("c192_ragged", (1, 192, 19, 33), 3213, False, 12, 2, (3e-06, 4.3e-06, 2.1e-05, 1.7e-05)),
    Sweep("c193", (1, 193, 16, 24), 3114, True, 16, 2, (1.1e-05, 1.9e-06, 7.9e-06, 2.4e-06)),
    Sweep("c256_b3", (3, 256, 16, 16), 3115, False, 16, 2, (2.7e-06, 2.7e-06, 1.4e-05, 3.3e-06)),
    Sweep("c120_n3337", (2, 120, 47, 71), 3116, False, 8, 4, (4.9e-06, 2.3e-06, 6.4e-05, 8e-06)),      # M = 40; the key pass is split
    Sweep("c120_n3337_signed", (2, 120, 47, 71), 3117, True, 8, 4, (2.8e-05, 1.2e-06, 1.7e-05, 1.7e-06)),
    Sweep("scale_312", (3, 20, 16, 24), 3118, False, 2, 2, (3.2e-06, 1.4e-06, 4.9e-06, 1.5e-06), scale=(3.0, 1.0, 2.0)),   # the maximum lies in sample 0
    Sweep("scale_123", (3, 20, 16, 24), 3219, False, 2, 2, (2.5e-06, 1.1e-06, 6.7e-06, 1.4e-06), scale=(1.0, 2.0, 3.0)),   # ... in the last sample
    Sweep("scale_123_signed", (3, 20, 16, 24), 3120, True, 2, 2, (1.1e-05, 1.2e-06, 7.8e-06, 7.2e-07), scale=(1.0, 2.0, 3.0)),
    Sweep("tie_zero", (1, 20, 16, 24), 3121, False, 2, 2, (2.8e-06, 9.5e-07, 2.5e-05, 1.6e-06), tie="zero"),         # lo = 0 is an M-way tie inside one query row
    Sweep("tie_zero_b2", (2, 20, 16, 24), 3122, False, 2, 2, (3.1e-06, 1.4e-06, 1.9e-05, 1.4e-06), tie="zero"),      # ... and across the two samples
    Sweep("tie_dup", (2, 12, 16, 16), 3123, False, 1, 2, (2.7e-06, 1.6e-06, 3.2e-05, 1.3e-06), tie="dup"),           # lo and hi both tie across the samples, bit for bit
    Sweep("limit_c256", (1, 256, 8, 8), 3124, False, 16, 2, (1.8e-06, 3.8e-06, 2.5e-06, 4.4e-06)),       # the entry limits that still launch: C = 256 at h = w = 8 ...
    Sweep("limit_8x15", (1, 1, 8, 15), 3125, False, 1, 2, (2.1e-06, 9e-07, 3e-06, 8.2e-07)),         # ... and ragged columns only, M = 1
]
BY_NAME = {c.name: c for c in SWEEP}
MUTANTS_A = ("uniform",)
MUTANTS_D = ("no_tB", "no_tC", "no_tD", "no_tR", "second")


def sweep_inputs(c):
    """(x, g) of a sweep case, float32: x = u^2 (u uniform) or standard normal, times the per-sample scale; g standard normal"""
    rng = np.random.default_rng(c.seed)
    x = rng.standard_normal(c.shape) if c.signed else rng.random(c.shape) ** 2
    g = rng.standard_normal(c.shape)
    x = x.astype(np.float32)
    if c.scale is not None:
        x *= np.asarray(c.scale, np.float32).reshape(-1, 1, 1, 1)
    if c.tie == "zero":
        x[:, :, ZERO_PIXEL // c.shape[3], ZERO_PIXEL % c.shape[3]] = 0
    if c.tie == "dup":
        x[1:] = x[:1]
    return x, g.astype(np.float32)


def _first_two(e, largest):
    """positions (b, i, j) of the extremum of E[B, N, M] and of the runner-up, first in C order among equals"""
    flat = (-e if largest else e).reshape(-1).copy()
    k0 = int(np.argmin(flat))
    if flat.size == 1:
        return np.unravel_index(k0, e.shape), None
    flat[k0] = np.inf
    return np.unravel_index(k0, e.shape), np.unravel_index(int(np.argmin(flat)), e.shape)


def _terms(x, g, dt):
    x, g = np.asarray(x, dt), np.asarray(g, dt)
    b, c, h, w = x.shape
    ph, pw = h // 8, w // 8
    n, m = h * w, ph * pw
    nchw = lambda t: t.transpose(0, 2, 1).reshape(b, c, h, w)       # [B, N, C] -> NCHW

    def up(dp):                                                      # pool8^T of [B, M, C] / 64 -> NCHW
        o = np.zeros((b, c, h, w), dt)
        o[:, :, :ph * 8, :pw * 8] = np.repeat(np.repeat(dp.transpose(0, 2, 1).reshape(b, c, ph, pw) * dt(1.0 / 64.0), 8, axis=2), 8, axis=3)
        return o

    xq = np.ascontiguousarray(x.reshape(b, c, n).transpose(0, 2, 1))
    gq = np.ascontiguousarray(g.reshape(b, c, n).transpose(0, 2, 1))
    p = x[:, :, :ph * 8, :pw * 8].reshape(b, c, ph, 8, pw, 8).sum(axis=(3, 5), dtype=dt) * dt(1.0 / 64.0)
    p = np.ascontiguousarray(p.reshape(b, c, m).transpose(0, 2, 1))
    pt = p.transpose(0, 2, 1)
    e = xq @ pt
    (plo, plo2), (phi, phi2) = _first_two(e, False), _first_two(e, True)
    lo, hi = e[plo], e[phi]
    r = dt(1.0) / (hi - lo)
    z = (e - lo) * r
    pe = np.exp(z)
    l = pe.sum(axis=2, dtype=dt)
    s = pe / l[:, :, None]
    a = s @ p
    y = a + xq                                                       # (rounded to dt: the kernels store y and the backward pass reads it)
    d = (gq * (y - xq)).sum(axis=2, keepdims=True, dtype=dt)
    dz = s * (gq @ pt - d)
    t = (dz * z).sum(dtype=dt)
    tb = r * (dz @ p)
    dpc = s.transpose(0, 2, 1) @ gq
    dpd = r * (dz.transpose(0, 2, 1) @ xq)

    def routed(pos_lo, pos_hi):
        tq, dp = np.zeros((b, n, c), dt), np.zeros((b, m, c), dt)
        for (bb, i, j), dv in ((pos_lo, r * t), (pos_hi, -(r * t))):
            tq[bb, i] += dv * p[bb, j]
            dp[bb, j] += dv * xq[bb, i]
        return nchw(tq) + up(dp)

    o = {"a": nchw(a), "y": nchw(y), "l": l, "lo": lo, "hi": hi, "r": r, "pos_lo": tuple(int(k) for k in plo), "pos_hi": tuple(int(k) for k in phi),
         "pos_lo2": tuple(int(k) for k in plo2), "pos_hi2": tuple(int(k) for k in phi2),
         "tB": nchw(tb), "tC": up(dpc), "tD": up(dpd), "tR": routed(plo, phi), "e": e}
    o["d"] = o["tB"] + o["tC"] + o["tD"] + o["tR"]
    o["gap_lo"], o["gap_hi"] = (e[plo2] - lo) * r, (hi - e[phi2]) * r     # (one key: the runner-up is another query's energy)
    if m > 1:
        o["a_uniform"] = nchw(np.broadcast_to(p.mean(axis=1, keepdims=True), (b, n, c)))
        o["tR_second"] = routed(plo2, phi2)
    return o


def nonlocal_terms_f64(x, g):
    """the term-wise float64 restatement: dict(a, y, l, lo, hi, r, pos_lo, pos_hi (b, i, j), the runners-up pos_lo2, pos_hi2, tB, tC, tD, tR, d = their sum, gap_lo, gap_hi, e) and,
    where M > 1, the material of the mutants: a_uniform (the softmax replaced by 1 / M) and tR_second (routed to the runners-up)"""
    return _terms(x, g, np.float64)


def nonlocal_terms_f32(x, g):
    """the same formulas in numpy float32 throughout: the yardstick of the sweep's tolerances"""
    return _terms(x, g, np.float32)


def mutants(c, ref):
    """name -> wrong-but-plausible value of a (MUTANTS_A) or d (MUTANTS_D).  M = 1 has S == 1 and dZ == 0: only "no_tC" is not structurally the truth"""
    if (c.shape[2] // 8) * (c.shape[3] // 8) == 1:
        return {"no_tC": ref["d"] - ref["tC"]}
    out = {"uniform": ref["a_uniform"], "second": ref["d"] - ref["tR"] + ref["tR_second"]}
    for k in ("tB", "tC", "tD", "tR"):
        out["no_" + k] = ref["d"] - ref[k]
    return out


def err_max(got, ref):
    """max |got - ref| / max |ref|  (a over the residual tensor, l over l)"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def err_d(d_got, ref, g):
    """the d norm: the smallest tol with |d_got - d_ref| <= 2^-23 |dx_ref| + tol max |d_ref| everywhere.  The first summand is the rounding of the
    stored dx and of the g + ... it was formed by, which d_got = dx - g cannot be better than; it is derived, not measured."""
    slack = 2.0 ** -23 * np.abs(np.asarray(g, np.float64) + ref["d"])
    return float(max(0.0, (np.abs(np.asarray(d_got, np.float64) - ref["d"]) - slack).max()) / np.abs(ref["d"]).max())


def err_energy(e, ref):
    """max |E - E_ref| / (hi - lo): the float32 yardstick of lo / hi / r.  lo and hi are two elements of E; the error of one given element is a
    lottery (it can be exactly 0), the maximum over the tensor is what an evaluation in another order can land on.  r = 1 / (hi - lo) then moves
    by at most twice that, relative to itself."""
    return float(np.abs(np.asarray(e, np.float64) - ref["e"]).max() / float(ref["hi"] - ref["lo"]))


def err_scalars(lo, hi, r, ref):
    """lo and hi relative to hi - lo, r relative to itself: the largest of the three"""
    span = float(ref["hi"] - ref["lo"])
    return max(abs(float(lo) - float(ref["lo"])) / span, abs(float(hi) - float(ref["hi"])) / span, abs(float(r) - float(ref["r"])) / float(ref["r"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, g, float64 terms, {mutant: its distance from the truth in the norm of its quantity}) of a sweep case, computed once and shared: read only"""
    c = BY_NAME[name]
    x, g = sweep_inputs(c)
    ref = nonlocal_terms_f64(x, g)
    dist = {k: (err_max(v, ref["a"]) if k in MUTANTS_A else err_d(v, ref, g)) for k, v in mutants(c, ref).items()}
    for a in (x, g, *(v for v in ref.values() if isinstance(v, np.ndarray))):
        a.setflags(write=False)
    return x, g, ref, dist


def float32_errors(name):
    """(a, l, d, lo/hi/r) errors of nonlocal_terms_f32 against the float64 terms, in the norms the GPU sweep uses.  a is taken the way the sweep has
    to take it, as the stored float32 y minus x, so the rounding of y (which grows with |x| / |a|: signed features) is part of the yardstick; d is
    the sum of the four float32 pieces, without g, because err_d already grants the rounding of the stored dx."""
    x, g, ref, _ = reference(name)
    f = nonlocal_terms_f32(x, g)
    assert f["pos_lo"] == ref["pos_lo"] and f["pos_hi"] == ref["pos_hi"], (name, "the float32 extrema sit elsewhere: the case is badly chosen")
    return (err_max(f["y"].astype(np.float64) - x, ref["a"]), err_max(f["l"], ref["l"]), err_max(f["d"], ref["d"]), err_energy(f["e"], ref))
