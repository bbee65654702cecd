"""Cases and numpy definitions of attention_fusion with the tensor-level poolings (reference core/fusion.py:32-126) and of SEDRFuse's fusion
strategy (reference core/model.py:271-281), for the kernels of csrc/attn_fuse.hip and golden F27.

evaluate(t1, t2, g, mode, sm, cm, dt) states every term in precision dt (float64: the definition; float32: the yardstick):
  s1, s2   spatial pools [n, h*w]:  'sum' | 'mean' | 'l1' | 'l2' | 'linf' over the channels, 'softmax_l1' = sum_c softmax_c(|x|) |x| (SEDRFuse)
  c1, c2   channel pools [n, c]:    'avg' | 'max' over the plane;  ci1, ci2: the row-major position of the maximum
  out      wf(a, b) = w t1 + (1 - w) t2, w = a / max(a + b, eps);  fs = wf(s1, s2), fc = wf(c1, c2);  'sa' fs, 'ca' fc, 'sca' (fs + fc) / 2,
           'wavg' w' fs + (1 - w') fc with w' = fs / max(fs + fc, eps)
  d1, d2   gradients of sum(out * g): the direct terms plus the terms through the pooled weights.
Sub-gradients as torch's CPU autograd takes them on the reference's ops: the clamp passes gradient where a + b >= eps (equality included); 'l1'
sign(x) with sign(0) = 0; 'l2' x / |x|_2 and 0 for a zero vector; 'linf' all to the FIRST channel holding the maximum; channel 'max' (max_pool2d
over the plane) all to the FIRST position in row-major order; 'softmax_l1' p_c (1 + |x_c| - s) sign(x_c).
tests/test_attn_fuse_oracle_cpu.py holds this definition to torch float64 autograd and to golden F27 (the reference's own code).

Inputs are rebuilt from seeds and are float32-exact, so that the fp32 kernels and the float64 definition start from the same numbers.
The error of a term is element-wise: max_i |got_i - ref_i| / max(|ref_i|, floor), floor = the median of |ref| (the largest |ref| where the median
is 0): an element is held relative to its own size or to the typical size of the term, whichever is larger.  Elements in the clamp's regime
(a + b < eps with a negative sum) reach 1e7 times the size of the others; a bound scaled by the largest element would hide all the rest.
The tolerance of a term is TOL_FACTOR x the error of the float32 evaluation of the same case and combination, and at least TOL_FACTOR ulps of
float32: in a case of a few elements the float32 evaluation can be exact by luck ('sum' over one channel, a maximum), while another correct
float32 order of operations (the kernels contract a * b + c) rounds the stored word differently.  All of it is computed on the CPU from the inputs
alone, nothing measured on the kernels.
"""
import dataclasses
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F27 = os.path.join(HERE, "golden", "f27_attn_fusion.npz")
EPS32 = np.float32(1e-7)
TOL_FACTOR = 8.0
ULP32 = 2.0 ** -23         # the yardstick's floor: two correct float32 evaluations in different operation orders differ by one ulp of a stored word
MUTANT_MARGIN = 20.0

MODES = ("sa", "ca", "sca", "wavg")
SPATIAL = ("sum", "mean", "l1", "l2", "linf")
SEDR = "softmax_l1"
CHANNEL = ("avg", "max")
MODE_CODE = {"sa": 0, "ca": 1, "sca": 2, "wavg": 3}
SPATIAL_CODE = {"sum": 0, "mean": 1, "l1": 2, "l2": 3, "linf": 4, SEDR: 5}
CHANNEL_CODE = {"avg": 0, "max": 1}
# the 5 x 2 x 4 public combinations + SEDRFuse's ('sa' with the internal pooling; the channel mode is not used)
COMBOS = tuple((m, s, c) for m in MODES for s in SPATIAL for c in CHANNEL) + (("sa", SEDR, "avg"),)
TERMS = ("s1", "s2", "c1", "c2", "out", "d1", "d2")


def uses(mode):
    """(spatial pools used, channel pools used)"""
    return mode != "ca", mode != "sa"


# ------------------------------------------------------------------------------------------------------------------------------ the definition
def _spatial(x, sm, dt, tie):
    """(s [n, 1, h, w], jac): jac(ds) = ds * ds/dx [n, c, h, w]"""
    c = x.shape[1]
    one = dt(1.0)
    if sm == "sum":
        return x.sum(axis=1, keepdims=True, dtype=dt), lambda ds: ds * np.ones_like(x)
    if sm == "mean":
        return x.sum(axis=1, keepdims=True, dtype=dt) / dt(c), lambda ds: (ds / dt(c)) * np.ones_like(x)
    if sm == "l1":
        return np.abs(x).sum(axis=1, keepdims=True, dtype=dt), lambda ds: ds * np.sign(x)
    if sm == "l2":
        s = np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=dt))
        safe = np.where(s > 0, s, one)
        return s, lambda ds: np.where(s > 0, x * (ds / safe), dt(0.0))
    if sm == "linf":
        s = x.max(axis=1, keepdims=True)
        hit = x == s
        if tie == "split":
            sel = hit / hit.sum(axis=1, keepdims=True, dtype=dt)
        else:
            k = np.argmax(hit, axis=1) if tie == "first" else c - 1 - np.argmax(hit[:, ::-1], axis=1)
            sel = np.arange(c).reshape(1, c, 1, 1) == k[:, None]
        return s, lambda ds: ds * sel.astype(dt)
    assert sm == SEDR, sm
    a = np.abs(x)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True, dtype=dt)
    s = (p * a).sum(axis=1, keepdims=True, dtype=dt)
    return s, lambda ds: ds * (p * (one + a - s)) * np.sign(x)


def _channel(x, cm, dt, tie, avg_as_sum):
    """(c [n, c, 1, 1], positions [n, c] or None, jac)"""
    n, c, h, w = x.shape
    flat = x.reshape(n, c, -1)
    if cm == "avg":
        if avg_as_sum:
            return flat.sum(axis=2, dtype=dt).reshape(n, c, 1, 1), None, lambda dc: dc * np.ones_like(x)
        return (flat.sum(axis=2, dtype=dt) / dt(h * w)).reshape(n, c, 1, 1), None, lambda dc: (dc / dt(h * w)) * np.ones_like(x)
    assert cm == "max", cm
    v = flat.max(axis=2, keepdims=True)
    hit = flat == v
    first = np.argmax(hit, axis=2)
    if tie == "split":
        sel = hit / hit.sum(axis=2, keepdims=True, dtype=dt)
        pos = first
    else:
        pos = first if tie == "first" else h * w - 1 - np.argmax(hit[:, :, ::-1], axis=2)
        sel = np.arange(h * w).reshape(1, 1, -1) == pos[:, :, None]
    return v.reshape(n, c, 1, 1), pos.astype(np.int32), lambda dc: dc * sel.astype(dt).reshape(x.shape)


def _wf(t1, t2, a, b, dt, eps, strict):
    """weighted_fusion and what its backward needs: torch's clamp passes gradient where a + b >= eps, equality included"""
    s = a + b
    den = np.maximum(s, eps)
    w = a / den
    return w * t1 + (dt(1.0) - w) * t2, w, den, (s > eps if strict else s >= eps)


def _wf_bwd(df, t1, t2, w, den, pas):
    dw = df * t1 - df * t2
    dden = np.where(pas, -dw * (w / den), 0.0).astype(dw.dtype)     # torch's div backward: -grad * ((self / other) / other)
    return dw / den + dden, dden


def evaluate(t1, t2, g, mode, sm, cm, dt=np.float64, eps=EPS32, mutant=None):
    """dict of TERMS + ci1, ci2 (None where the mode has no such term) in precision dt.  eps: the kernels' and float32 torch's clamp is
    float32(1e-7); float64 torch clamps at the double 1e-7.  mutant: one of MUTANTS, a wrong-but-plausible variant."""
    assert mutant is None or mutant in MUTANTS, mutant
    eps = dt(eps)
    t1, t2, g = (np.asarray(t, dt) for t in (t1, t2, g))
    n, c, h, w = t1.shape
    if mutant == "wavg_as_sca" and mode == "wavg":
        mode = "sca"
    if mutant == "mean_as_sum" and sm == "mean":
        sm = "sum"
    if mutant == "l2_as_l1" and sm == "l2":
        sm = "l1"
    tie = {"tie_split": "split", "tie_last": "last"}.get(mutant, "first")
    strict = mutant == "clamp_strict"
    sp, ch = uses(mode)
    o = dict.fromkeys(TERMS + ("ci1", "ci2"))
    if sp:
        s1, j1 = _spatial(t1, sm, dt, tie)
        s2, j2 = _spatial(t2, sm, dt, tie)
        o["s1"], o["s2"] = s1.reshape(n, -1), s2.reshape(n, -1)
        if mutant == "swap_s":
            s1, s2 = s2, s1
        fs, ws, dens, ps = _wf(t1, t2, s1, s2, dt, eps, strict)
    if ch:
        c1, o["ci1"], k1 = _channel(t1, cm, dt, tie, mutant == "avg_as_sum")
        c2, o["ci2"], k2 = _channel(t2, cm, dt, tie, mutant == "avg_as_sum")
        o["c1"], o["c2"] = c1.reshape(n, c), c2.reshape(n, c)
        fc, wc, denc, pc = _wf(t1, t2, c1, c2, dt, eps, strict)
    if mode == "sa":
        out, dfs = fs, g
    elif mode == "ca":
        out, dfc = fc, g
    elif mode == "sca":
        out = (fs + fc) / dt(2.0)
        dfs = dfc = g / dt(2.0)
    else:
        out, wo, deno, po = _wf(fs, fc, fs, fc, dt, eps, strict)
        da, db = _wf_bwd(g, fs, fc, wo, deno, po)
        dfs, dfc = g * wo + da, g * (dt(1.0) - wo) + db
    d1, d2 = np.zeros_like(t1), np.zeros_like(t1)
    pooled = mutant != "no_pool_grad"
    if sp:
        das, dbs = _wf_bwd(dfs, t1, t2, ws, dens, ps)
        d1, d2 = d1 + dfs * ws, d2 + dfs * (dt(1.0) - ws)
        if pooled:
            das, dbs = das.sum(axis=1, keepdims=True, dtype=dt), dbs.sum(axis=1, keepdims=True, dtype=dt)
            if mutant == "swap_s":
                das, dbs = dbs, das
            d1, d2 = d1 + j1(das), d2 + j2(dbs)
    if ch:
        dac, dbc = _wf_bwd(dfc, t1, t2, wc, denc, pc)
        d1, d2 = d1 + dfc * wc, d2 + dfc * (dt(1.0) - wc)
        if pooled:
            d1 = d1 + k1(dac.sum(axis=(2, 3), keepdims=True, dtype=dt))
            d2 = d2 + k2(dbc.sum(axis=(2, 3), keepdims=True, dtype=dt))
    o["out"], o["d1"], o["d2"] = out, d1, d2
    return o


MUTANTS = ("no_pool_grad", "mean_as_sum", "avg_as_sum", "l2_as_l1", "tie_split", "tie_last", "clamp_strict", "wavg_as_sca", "swap_s")


# ------------------------------------------------------------------------------------------------------------------------------ the norm
def err(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    mag = np.abs(ref)
    top = mag.max()
    diff = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    if top == 0.0:
        return 0.0 if diff.max() == 0.0 else float("inf")
    floor = np.median(mag)
    if floor == 0.0:
        floor = top
    return float((diff / np.maximum(mag, floor)).max())


def errors(got, ref):
    """{term: error} over the terms the combination has"""
    return {k: err(got[k], ref[k]) for k in TERMS if ref[k] is not None}


# ------------------------------------------------------------------------------------------------------------------------------ the cases
@dataclasses.dataclass(frozen=True)
class Case:
    """kind: "pos" non-negative features (like post-ReLU maps), "signed" (every 7th pixel vector moved down by 1 in t1 and by 3 in t2: clearly negative sums there, which exercise the clamp, clearly positive ones elsewhere),
    "eps" (pools planted below, on and above the clamp).  ties: plant_ties.  combos: the combinations run (None: all of COMBOS).
    offset: the sweep shifts every device pointer by this many floats (breaks 16-byte alignment of the base)"""
    name: str
    shape: tuple
    seed: int
    kind: str = "pos"
    ties: bool = False
    combos: tuple = None
    offset: int = 0


SOME = (("wavg", "l2", "max"), ("sca", "mean", "avg"), ("sa", "linf", "avg"), ("ca", "l1", "max"), ("wavg", "l1", "avg"), ("sa", SEDR, "avg"))
# signed features only where the CPU test shows the float32 evaluation to be well conditioned: 'wavg' (fs + fc near 0) and the norms stay out
SIGNED = (("sa", "sum", "avg"), ("sca", "sum", "avg"), ("sa", "mean", "avg"), ("sca", "mean", "max"), ("ca", "sum", "avg"))

CASES = [
    Case("n1c1_1x1", (1, 1, 1, 1), 2701),
    Case("n2c2_1x63", (2, 2, 1, 63), 2702),
    Case("n1c3_8x8", (1, 3, 8, 8), 2703),
    Case("n3c16_5x13", (3, 16, 5, 13), 2704),                       # 65 pixels: rows off 16-byte alignment
    Case("n2c17_15x17", (2, 17, 15, 17), 2705),                     # 255
    Case("n1c257_257x1", (1, 257, 257, 1), 2706, combos=SOME),
    Case("n2c3_25x40", (2, 3, 25, 40), 2707),                       # 1000: the 16-byte path with a ragged tile
    Case("n2c3_25x40_off1", (2, 3, 25, 40), 2707, offset=1, combos=SOME),
    Case("n2c5_7x9_ties", (2, 5, 7, 9), 2708, ties=True),
    Case("n3c2_33x37", (3, 2, 33, 37), 2709, combos=SOME),          # 1221: two tiles, scalar path
    Case("n1c2_300x300", (1, 2, 300, 300), 2710, combos=SOME),      # 88 tiles: several blocks per channel sum
    Case("pool_cap", (1030, 2, 3, 1), 2711, combos=SOME),           # more (sample, tile, chunk) items than the channel-walking kernels' grid cap (1024)
    Case("n2c40_64x65", (2, 40, 64, 65), 2717, combos=SOME),        # 5 tiles of 5 chunks of 8 channels: chunks and tiles together
    Case("elem_cap", (17, 257, 1, 3), 2712, combos=SOME),           # more (sample, channel, tile) items than the element-wise cap (4096)
    Case("eps", (3, 4, 8, 8), 2713, kind="eps"),
    Case("signed", (2, 3, 25, 40), 2714, kind="signed", combos=SIGNED),
    Case("plane_1224x1024", (1, 1, 1224, 1024), 2715, combos=(("ca", "l1", "avg"),)),
    Case("gold", (2, 3, 3, 4), 2716, ties=True),                    # the case of golden F27
]
BY_NAME = {c.name: c for c in CASES}
POOL_GRID_CAP, ELEM_GRID_CAP, TILE = 1024, 4096, 1024
ITEMS, MIN_CHUNK = 64, 8


def chunks_for(c, npx):
    """mirror of af_check in csrc/attn_fuse.hip: (channel chunks K of the channel-walking kernels, channels per chunk) -- of (c, h * w) alone"""
    tiles = -(-npx // TILE)
    want = min(-(-ITEMS // tiles), -(-c // MIN_CHUNK))
    cpc = -(-c // want)
    return -(-c // cpc), cpc

# every mutant, and the cases and combinations built to show it
MUTANT_CASES = {
    "no_pool_grad": [("n2c5_7x9_ties", cb) for cb in COMBOS],
    "mean_as_sum": [("n3c16_5x13", ("sa", "mean", "avg")), ("n3c16_5x13", ("wavg", "mean", "max"))],
    "avg_as_sum": [("n3c16_5x13", ("ca", "l1", "avg")), ("n3c16_5x13", ("wavg", "l2", "avg"))],
    "l2_as_l1": [("n3c16_5x13", ("sa", "l2", "avg")), ("n3c16_5x13", ("sca", "l2", "max"))],
    "tie_split": [("n2c5_7x9_ties", ("sa", "linf", "avg")), ("n2c5_7x9_ties", ("ca", "l1", "max")), ("gold", ("wavg", "linf", "max"))],
    "tie_last": [("n2c5_7x9_ties", ("sa", "linf", "avg")), ("n2c5_7x9_ties", ("ca", "l1", "max")), ("gold", ("wavg", "linf", "max"))],
    "clamp_strict": [("eps", ("sa", "sum", "avg")), ("eps", ("sa", "l1", "avg")), ("eps", ("sa", "l2", "avg")), ("eps", ("sa", "linf", "avg")),
                     ("eps", ("sa", "mean", "avg")), ("eps", ("ca", "l1", "max")), ("eps", ("ca", "l1", "avg"))],
    "wavg_as_sca": [("n3c16_5x13", cb) for cb in COMBOS if cb[0] == "wavg"],
    "swap_s": [("n3c16_5x13", cb) for cb in COMBOS if cb[0] != "ca"],
}

# "eps": where the planted sums sit.  Pairs (a, b) with a + b just below / exactly on / just above float32(1e-7), each sum exact in float32:
_A = np.float32(2.0 ** -24)
EPS_PAIRS = ((_A, np.nextafter(EPS32, np.float32(0)) - _A), (_A, EPS32 - _A), (_A, np.nextafter(EPS32, np.float32(1)) - _A))


def plant_ties(x1, x2):
    """two channels sharing a pixel's maximum, a plane maximum at three positions, all-zero pixel vectors (in both tensors: s1 + s2 = 0) and an
    all-zero plane (in both: c1 + c2 = 0, the maximum at element 0)"""
    n, c, h, w = x1.shape
    f1, f2 = x1.reshape(n, c, -1), x2.reshape(n, c, -1)
    npx = h * w
    for f in (f1, f2):
        f[0, c - 1, :] = 0.0                                    # an all-zero plane
        f[:, :, npx - 1] = 0.0                                  # all-zero pixel vectors (the last pixel of every sample)
        f[n - 1, 0, [1, npx // 2, npx - 2]] = 2.0               # the plane maximum at three positions
        f[0, [0, c - 2], 3] = 1.5                               # two channels share pixel 3's maximum
        f[n - 1, :, 5] = f[n - 1, 0, 5]                         # ... and every channel pixel 5's


def plant_eps(x1, x2):
    """sample 0: pixels 0-2 carry the EPS_PAIRS in channel 0 and zeros elsewhere ('sum', 'l1', 'l2', 'linf' pools land below / on / above the clamp
    exactly), pixels 3-5 the same times C (exact for 'mean' when C is a power of two); sample 1: planes 0-2 are zero but for element 5 (exact
    for 'max'); sample 2: the same times h * w (exact for 'avg' when h * w is a power of two).  Everything else is ordinary."""
    n, c, h, w = x1.shape
    f1, f2 = x1.reshape(n, c, -1), x2.reshape(n, c, -1)
    for k, (a, b) in enumerate(EPS_PAIRS):
        for f, v in ((f1, a), (f2, b)):
            f[0, :, k] = 0.0
            f[0, 0, k] = v
            f[0, :, 3 + k] = 0.0
            f[0, 0, 3 + k] = v * np.float32(c)
            f[1, k, :] = 0.0
            f[1, k, 5] = v
            f[2, k, :] = 0.0
            f[2, k, 5] = v * np.float32(h * w)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(t1, t2, upstream) of a case, float32, read-only"""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    x1, x2 = (rng.random(c.shape) ** 2).astype(np.float32), (rng.random(c.shape) ** 2).astype(np.float32)
    g = rng.standard_normal(c.shape).astype(np.float32)
    if c.kind == "signed":
        for x, shift in ((x1, 1.0), (x2, 3.0)):      # (apart by more than 1: w t1 + (1 - w) t2 with |w| ~ 1e7 does not cancel)
            x.reshape(c.shape[0], c.shape[1], -1)[:, :, 3::7] -= np.float32(shift)
    if c.kind == "eps":
        plant_eps(x1, x2)
    if c.ties:
        plant_ties(x1, x2)
    for a in (x1, x2, g):
        a.setflags(write=False)
    return x1, x2, g


def combos(c):
    return COMBOS if c.combos is None else c.combos


@functools.lru_cache(maxsize=None)
def reference(name, combo):
    """(float64 definition, {term: tolerance}) of a case and combination, computed once and shared: read only"""
    t1, t2, g = inputs(name)
    ref = evaluate(t1, t2, g, *combo, dt=np.float64)
    f32 = evaluate(t1, t2, g, *combo, dt=np.float32)
    for k in ("ci1", "ci2"):
        assert (ref[k] is None and f32[k] is None) or np.array_equal(ref[k], f32[k]), (name, combo, k)
    tol = {k: TOL_FACTOR * max(v, ULP32) for k, v in errors(f32, ref).items()}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref, tol


def mutant_margin(name, combo, mutant):
    """the largest distance of the mutant from the definition over the terms, in tolerances of that term (inf: a term the float32 evaluation gets
    exactly, or a position, differs)"""
    t1, t2, g = inputs(name)
    ref, tol = reference(name, combo)
    mut = evaluate(t1, t2, g, *combo, dt=np.float64, mutant=mutant)
    best = 0.0
    for k, d in errors(mut, ref).items():
        if d > 0.0:
            best = max(best, d / tol[k] if tol[k] > 0.0 else float("inf"))
    for k in ("ci1", "ci2"):
        if ref[k] is not None and not np.array_equal(ref[k], mut[k]):
            best = float("inf")
    return best
