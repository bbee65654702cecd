"""Cases and numpy float64 restatements of channel_pooling(x, 'nl') (reference core/fusion.py:137-150) and of the join of
attention_fusion(a, b, mode, 'nl', 'nl') (:32-59) for golden F26.

The fixture tests/golden/f26_channel_nl.npz (written by tests/golden/make_golden_channel_nl.py from the reference's own code in float64)
holds results only; the inputs are rebuilt here from seeds and are float32-exact, so that the fp32 kernels and the float64 oracles start
from the same numbers.  Gradients are those of sum(y * upstream(case)).  Arrays of more than SAMPLE_ABOVE elements are stored at
sample_index(size).

With X = x.reshape(B, C, N):  E = X X^T,  lo / hi = min / max of E over all of (B, C, C),  r = 1 / (hi - lo),  Z = (E - lo) r,
A = softmax_rows(Z),  y = A X + x;  for upstream G:  dA = G X^T,  D_i = sum_j dA_ij A_ij,  dZ = A o (dA - D),  T = sum dZ o Z (whole batch),
M = r dZ + r T at the argmin element of E - r T at the argmax element,  dx = g + A^T G + (M + M^T) X.
E is symmetric, so an off-diagonal extremum ties with its transpose twin; (M + M^T) makes the choice between the twins immaterial.  Other
ties go to the first element in C order of E[B, C, C] (np.argmin / np.argmax): the kernels' documented rule, not torch's even split.

The second half is the table of tests/test_gpu_channel_nl_sweep.py: SWEEP, the term-wise float64 restatement (channel_terms_f64, whose pieces sum
to channel_f64), the float32 yardstick (the same formulas in float32, evaluated twice: numpy's blocked matmul, and the two N-long contractions
accumulated strictly sequentially in steps of 4 positions, the matrix instruction's K step; per quantity the larger error counts), the mutants,
and the join's float64 definition with torch's clamp rule.
"""
import dataclasses
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F26 = os.path.join(HERE, "golden", "f26_channel_nl.npz")
SAMPLE_ABOVE = 6000
MIN_GAP = 1e-4        # non-tie cases: both extremum gaps (twin ignored) are at least this fraction of hi - lo ...
GAP_OVER_ERR = 100.0  # ... and this many float32 energy errors

# model-level cases: name -> (shape, seed, signed, per-sample scale)
CASES = {
    "b2c7": ((2, 7, 5, 9), 2601, False, None),
    "c20_signed": ((1, 20, 16, 24), 2602, True, None),
    "b3c1": ((3, 1, 4, 4), 2603, False, None),
    "c112": ((1, 112, 16, 24), 2604, False, None),
    "scale2": ((2, 12, 16, 24), 2605, False, (1.0, 3.0)),
}
FUSION_SHAPE, FUSION_SEED = (2, 12, 16, 16), 2650
FUSION_MODES = ("sa", "ca", "sca", "wavg")
EPS32 = np.float32(1e-7)


def _draw(shape, seed, signed, scale):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) if signed else rng.random(shape) ** 2).astype(np.float32)
    if scale is not None:
        x *= np.asarray(scale, np.float32).reshape(-1, 1, 1, 1)
    return x


def inputs(name):
    shape, seed, signed, scale = CASES[name]
    return _draw(shape, seed, signed, scale)


def upstream(name):
    shape, seed, _, _ = CASES[name]
    return np.random.default_rng(seed + 5000).standard_normal(shape).astype(np.float32)


def fusion_inputs():
    """(t1, t2, upstream) of the fusion-layer case: non-negative features, like post-ReLU maps"""
    return (_draw(FUSION_SHAPE, FUSION_SEED, False, None), _draw(FUSION_SHAPE, FUSION_SEED + 1, False, None),
            np.random.default_rng(FUSION_SEED + 2).standard_normal(FUSION_SHAPE).astype(np.float32))


def sample_index(size):
    if size <= SAMPLE_ABOVE:
        return np.arange(size)
    k = -(-size // SAMPLE_ABOVE) | 1
    return np.arange(0, size, k)


# ------------------------------------------------------------------------------------------------------------------------------ geometry mirror
KC_SET = (1, 2, 4, 7, 8, 12, 16)
CHUNK_BLOCKS = 256


def kc_for(c):
    """mirror of nlc_kc_for in csrc/nonlocal_channel.hip: the 16-channel tiles the kernels run for C channels"""
    need = (c + 15) // 16
    return next(k for k in KC_SET if k >= need)


def kc_range(kc):
    """lowest and highest C that run on KC tiles"""
    i = KC_SET.index(kc)
    return (KC_SET[i - 1] * 16 + 1 if i else 1), kc * 16


def chunk_cap(b):
    """mirror of nlc_make_geo: the gram pass cuts N into at most this many chunks per sample"""
    return max(1, CHUNK_BLOCKS // b)


def chunks_for(b, n):
    """(64-position tiles, chunks per sample, tiles per chunk)"""
    tiles = (n + 63) // 64
    want = min(tiles, chunk_cap(b))
    tpc = -(-tiles // want)
    return tiles, -(-tiles // tpc), tpc


# ------------------------------------------------------------------------------------------------------------------------------ the definition
def _gram(a, b, dt, seq):
    """a b^T over the last axis of [B, C, N] operands; seq: accumulated strictly sequentially in steps of 4 positions"""
    if not seq:
        return a @ b.transpose(0, 2, 1)
    acc = np.zeros((a.shape[0], a.shape[1], b.shape[1]), dt)
    for k in range(0, a.shape[2], 4):
        acc += a[:, :, k:k + 4] @ b[:, :, k:k + 4].transpose(0, 2, 1)
    return acc


def _first_two(e, largest):
    """positions (b, i, j) of the extremum of E[B, C, C] and of the runner-up, first in C order among equals; the runner-up ignores the
    extremum's transpose twin"""
    flat = (-e if largest else e).reshape(-1).copy()
    k0 = int(np.argmin(flat))
    p0 = tuple(int(k) for k in np.unravel_index(k0, e.shape))
    flat[k0] = np.inf
    flat[np.ravel_multi_index((p0[0], p0[2], p0[1]), e.shape)] = np.inf
    if not np.isfinite(flat).any():
        return p0, None
    return p0, tuple(int(k) for k in np.unravel_index(int(np.argmin(flat)), e.shape))


def _terms(x, g, dt, seq=False):
    x4, g4 = np.asarray(x, dt), np.asarray(g, dt)
    b, c, h, w = x4.shape
    X, G = x4.reshape(b, c, -1), g4.reshape(b, c, -1)
    e = _gram(X, X, dt, seq)
    e = np.triu(e) + np.triu(e, 1).transpose(0, 2, 1)              # one triangle, mirrored: symmetric bit for bit in every precision
    (plo, plo2), (phi, phi2) = _first_two(e, False), _first_two(e, True)
    lo, hi = e[plo], e[phi]
    r = dt(1.0) / (hi - lo)
    z = (e - lo) * r
    pe = np.exp(z)
    attn = pe / pe.sum(axis=2, keepdims=True, dtype=dt)
    a = attn @ X
    y = a + X                                                       # (rounded to dt: the kernels store y)
    da = _gram(G, X, dt, seq)
    d_ = (da * attn).sum(axis=2, keepdims=True, dtype=dt)
    dz = attn * (da - d_)
    t = (dz * z).sum(dtype=dt)
    ta = attn.transpose(0, 2, 1) @ G
    tb = (r * dz + r * dz.transpose(0, 2, 1)) @ X

    def routed(pos_lo, pos_hi):
        o = np.zeros((b, c, X.shape[2]), dt)
        for (bb, i, j), dv in ((pos_lo, r * t), (pos_hi, -(r * t))):
            o[bb, i] += dv * X[bb, j]
            o[bb, j] += dv * X[bb, i]
        return o

    sh = (b, c, h, w)
    o = {"a": a.reshape(sh), "y": y.reshape(sh), "e": e, "attn": attn, "lo": lo, "hi": hi, "r": r, "pos_lo": plo, "pos_hi": phi, "pos_lo2": plo2,
         "pos_hi2": phi2, "tA": ta.reshape(sh), "tB": tb.reshape(sh), "tR": routed(plo, phi).reshape(sh), "t": t}
    o["d"] = o["tA"] + o["tB"] + o["tR"]
    if plo2 is not None:
        o["gap_lo"], o["gap_hi"] = (e[plo2] - lo) * r, (hi - e[phi2]) * r
        o["tR_second"] = routed(plo2, phi2).reshape(sh)
    if c > 1:
        o["a_uniform"] = np.broadcast_to(X.mean(axis=1, keepdims=True), X.shape).reshape(sh)
    return o


def channel_terms_f64(x, g):
    """the term-wise float64 restatement: dict(a = A X, y, e, attn, lo, hi, r, pos_lo, pos_hi (b, i, j), the runners-up pos_lo2 / pos_hi2 (twin
    ignored), tA = A^T G, tB = (r dZ + r dZ^T) X, tR (the routed terms), d = their sum, gap_lo, gap_hi) and the material of the mutants:
    a_uniform (the softmax replaced by 1 / C) and tR_second (routed to the runners-up)"""
    return _terms(x, g, np.float64)


def channel_terms_f32(x, g, seq):
    """the same formulas in numpy float32 throughout; seq: the two N-long contractions in the matrix instruction's order"""
    return _terms(x, g, np.float32, seq)


def channel_f64(x, g=None):
    """float64 restatement, written independently of _terms: dict(y, dx (if g), lo, hi)"""
    x = np.asarray(x, np.float64)
    b, c, h, w = x.shape
    X = x.reshape(b, c, -1)
    e = np.einsum("bin,bjn->bij", X, X)
    lo, hi = e.min(), e.max()
    r = 1.0 / (hi - lo)
    z = (e - lo) * r
    pe = np.exp(z)
    A = pe / pe.sum(axis=2, keepdims=True)
    out = {"y": (A @ X + X).reshape(x.shape), "lo": lo, "hi": hi}
    if g is None:
        return out
    G = np.asarray(g, np.float64).reshape(b, c, -1)
    dA = G @ X.transpose(0, 2, 1)
    dZ = A * (dA - (dA * A).sum(axis=2, keepdims=True))
    T = (dZ * z).sum()
    M = r * dZ
    M[np.unravel_index(np.argmin(e), e.shape)] += r * T
    M[np.unravel_index(np.argmax(e), e.shape)] -= r * T
    out["dx"] = (G + A.transpose(0, 2, 1) @ G + (M + M.transpose(0, 2, 1)) @ X).reshape(x.shape)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ norms
def err_el(got, ref, stored, bits=24):
    """the smallest tol with |got - ref| <= 2^-bits |stored| + tol max |ref| everywhere.  The first summand is the rounding of the float32 word the
    value was read from (`stored`: its float64 value); it is derived, not measured."""
    ref = np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    excess = (np.abs(np.asarray(got, np.float64) - ref) - 2.0 ** -bits * np.abs(stored)).max()
    if top == 0.0:
        return 0.0 if excess <= 0.0 else float("inf")
    return float(max(0.0, excess) / top)


def err_a(y_got, x, ref):
    """a = y - x against A X: over the attention term, not over y, which x dominates; y is the stored word"""
    return err_el(np.asarray(y_got, np.float64) - x, ref["a"], ref["y"])


def err_d(dx_got, g, ref):
    """d = dx - g against tA + tB + tR; the stored dx is g + d, rounded once for the sum and once for the word"""
    return err_el(np.asarray(dx_got, np.float64) - g, ref["d"], np.asarray(g, np.float64) + ref["d"], bits=23)


def err_e(e, ref):
    return err_el(e, ref["e"], ref["e"])


def err_attn(attn, ref):
    return err_el(attn, ref["attn"], ref["attn"])


def err_scalars(lo, hi, r, e, ref):
    """lo and hi relative to hi - lo, r relative to itself; the yardstick of all three is the largest energy error relative to hi - lo (lo and hi are
    two elements of E, and the error of one given element is a lottery), r moving by at most twice that"""
    span = float(ref["hi"] - ref["lo"])
    if e is not None:                                               # the yardstick side
        return float(np.abs(np.asarray(e, np.float64) - ref["e"]).max() / span)
    return max(abs(float(lo) - float(ref["lo"])) / span, abs(float(hi) - float(ref["hi"])) / span, 0.5 * abs(float(r) - float(ref["r"])) / float(ref["r"]))


QUANTITIES = ("e", "attn", "scalars", "a", "d")


# ------------------------------------------------------------------------------------------------------------------------------ the sweep
@dataclasses.dataclass(frozen=True)
class Sweep:
    """kc is what the case claims to exercise, checked against kc_for.  tie: "zero" = channel ZERO_CHANNEL of every sample is 0 (lo = 0 ties across a
    whole row and column of E); "dup" = sample 1 is a bit-copy of sample 0"""
    name: str
    shape: tuple
    seed: int
    signed: bool
    kc: int
    scale: tuple = None
    tie: str = None


ZERO_CHANNEL = 7

SWEEP = [
    Sweep("c1_n1", (2, 1, 1, 1), 4101, False, 1),                    # n * c = 2: the smallest legal call; A == 1, dZ == 0
    Sweep("c2_n15", (1, 2, 3, 5), 4102, True, 1),                    # n * c = 2 with one sample
    Sweep("c15_n3", (1, 15, 1, 3), 4103, False, 1),
    Sweep("c16_n5", (1, 16, 5, 1), 4104, False, 1),
    Sweep("c17_n63", (2, 17, 7, 9), 4105, False, 2),
    Sweep("c32_n64", (1, 32, 8, 8), 4106, True, 2),
    Sweep("c33_n65", (1, 33, 5, 13), 4107, False, 4),
    Sweep("c64_ragged", (2, 64, 33, 65), 4108, True, 4),             # N = 2145 = 33 * 64 + 33: 34 tiles, 34 chunks
    Sweep("c65", (1, 65, 7, 9), 4109, False, 7),
    Sweep("c112", (2, 112, 16, 24), 4110, False, 7),
    Sweep("c113", (1, 113, 7, 9), 4111, True, 8),
    Sweep("c128", (1, 128, 8, 24), 4112, False, 8),
    Sweep("c129", (1, 129, 4, 16), 4113, True, 12),                  # two row groups in the gram pass
    Sweep("c192", (1, 192, 5, 7), 4114, False, 12),
    Sweep("c193", (1, 193, 8, 8), 4115, True, 16),
    Sweep("c256_b3", (3, 256, 8, 8), 4116, False, 16),
    Sweep("chunks_over_cap", (8, 20, 33, 65), 4117, False, 2),       # 34 tiles against a cap of 32 chunks: two tiles per chunk
    Sweep("scale_312", (3, 20, 16, 24), 4118, False, 2, scale=(3.0, 1.0, 2.0)),    # the maximum lies in sample 0
    Sweep("scale_123", (3, 20, 16, 24), 4119, False, 2, scale=(1.0, 2.0, 3.0)),    # ... in the last sample
    Sweep("scale_123_signed", (3, 20, 16, 24), 4120, True, 2, scale=(1.0, 2.0, 3.0)),
    Sweep("tie_zero", (2, 20, 16, 24), 4121, False, 2, tie="zero"),
    Sweep("tie_dup", (2, 12, 16, 16), 4122, False, 1, tie="dup"),
    Sweep("limit_c256_n1", (1, 256, 1, 1), 4123, True, 16),          # E = x x^T, one position
]
BY_NAME = {c.name: c for c in SWEEP}
MUTANTS_A = ("uniform",)
MUTANTS_D = ("no_tA", "no_tB", "no_tR", "second")
TOL_FACTOR = 8.0      # the kernels sum in another order than either float32 evaluation (64-position tiles, chunks) and use expf
MUTANT_MARGIN = 20.0


def sweep_inputs(c):
    rng = np.random.default_rng(c.seed)
    x = (rng.standard_normal(c.shape) if c.signed else rng.random(c.shape) ** 2).astype(np.float32)
    g = rng.standard_normal(c.shape).astype(np.float32)
    if c.scale is not None:
        x *= np.asarray(c.scale, np.float32).reshape(-1, 1, 1, 1)
    if c.tie == "zero":
        x[:, ZERO_CHANNEL] = 0
    if c.tie == "dup":
        x[1:] = x[:1]
    return x, g


def mutants(c, ref):
    """name -> wrong-but-plausible value of a (MUTANTS_A) or d (MUTANTS_D).  C = 1 has A == 1 and dZ == 0: only "no_tA" is not structurally the truth"""
    out = {"no_tA": ref["d"] - ref["tA"]}
    if c.shape[1] > 1:
        out["uniform"] = ref["a_uniform"]
        out["no_tB"] = ref["d"] - ref["tB"]
        out["no_tR"] = ref["d"] - ref["tR"]
        out["second"] = ref["d"] - ref["tR"] + ref["tR_second"]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, g, float64 terms, {mutant: its distance from the truth in the norm of its quantity}) of a sweep case, computed once and shared: read only"""
    c = BY_NAME[name]
    x, g = sweep_inputs(c)
    ref = channel_terms_f64(x, g)
    dist = {}
    for k, v in mutants(c, ref).items():
        dist[k] = err_el(v, ref["a"], ref["y"]) if k in MUTANTS_A else err_el(v, ref["d"], g.astype(np.float64) + ref["d"], bits=23)
    for a in (x, g, *(v for v in ref.values() if isinstance(v, np.ndarray))):
        a.setflags(write=False)
    return x, g, ref, dist


@functools.lru_cache(maxsize=None)
def float32_errors(name):
    """{quantity: error} of the float32 evaluations against the float64 terms, in the norms the GPU sweep uses: per quantity the larger of the
    blocked and the sequential evaluation.  a is taken the way the sweep takes it, as the stored float32 y minus x."""
    x, g, ref, _ = reference(name)
    out = dict.fromkeys(QUANTITIES, 0.0)
    for seq in (False, True):
        f = channel_terms_f32(x, g, seq)
        assert f["pos_lo"] == ref["pos_lo"] and f["pos_hi"] == ref["pos_hi"], (name, "the float32 extrema sit elsewhere: the case is badly chosen")
        figs = {"e": err_e(f["e"], ref), "attn": err_attn(f["attn"], ref), "scalars": err_scalars(None, None, None, f["e"], ref),
                "a": err_a(f["y"], x, ref), "d": err_d(g.astype(np.float64) + f["d"], g, ref)}
        out = {k: max(out[k], figs[k]) for k in QUANTITIES}
    return out


def tolerances(name):
    """{quantity: TOL_FACTOR x the float32 yardstick}: computed on the CPU from the case alone, nothing measured on the kernels"""
    return {k: TOL_FACTOR * v for k, v in float32_errors(name).items()}


# ------------------------------------------------------------------------------------------------------------------------------ the join
JOIN_MODES = {"sa": 0, "ca": 1, "sca": 2, "wavg": 3}
JOIN_COUNTS = (1, 255, 256, 257, 4096 * 256 + 77)      # around the block size, and past the grid cap (4096 blocks of 256: grid-stride)
JOIN_GRID_CAP = 4096
PLANTED = 4                                             # clamp-regime elements planted at the head of every join case


def _wf(t1, t2, a, b, dt, eps):
    """weighted_fusion and the pieces its backward needs: torch's clamp passes gradient where a + b >= eps, equality included"""
    s = a + b
    den = np.maximum(s, eps)
    w = a / den
    return w * t1 + (dt(1.0) - w) * t2, w, den, s >= eps


def _wf_bwd(df, t1, t2, w, den, pas):
    dw = df * t1 - df * t2
    dden = np.where(pas, -dw * (w / den), 0.0).astype(dw.dtype)      # torch's div backward: -grad * ((self / other) / other)
    return dw / den + dden, dden


def join_def(mode, t1, t2, s1, s2, c1, c2, g=None, dt=np.float64, eps=EPS32):
    """the join in precision dt: out, and for upstream g the six gradients (None where the mode has no such map).  eps: the kernels' and float32
    torch's clamp is float32(1e-7); float64 torch clamps at the double 1e-7 (the CPU pin passes that)"""
    eps = dt(eps)
    cv = lambda t: None if t is None else np.asarray(t, dt)
    t1, t2, s1, s2, c1, c2, g = (cv(t) for t in (t1, t2, s1, s2, c1, c2, g))
    sp, ch = mode != "ca", mode != "sa"
    if sp:
        fs, ws, dens, ps = _wf(t1, t2, s1, s2, dt, eps)
    if ch:
        fc, wc, denc, pc = _wf(t1, t2, c1, c2, dt, eps)
    if mode == "sa":
        out = fs
    elif mode == "ca":
        out = fc
    elif mode == "sca":
        out = (fs + fc) / dt(2.0)
    else:
        out, wo, deno, po = _wf(fs, fc, fs, fc, dt, eps)
    if g is None:
        return out
    dfs = dfc = None
    if mode == "sa":
        dfs = g
    elif mode == "ca":
        dfc = g
    elif mode == "sca":
        dfs = dfc = g / dt(2.0)
    else:
        da, db = _wf_bwd(g, fs, fc, wo, deno, po)
        dfs, dfc = g * wo + da, g * (dt(1.0) - wo) + db
    d1, d2 = np.zeros_like(t1), np.zeros_like(t1)
    ds1 = ds2 = dc1 = dc2 = None
    if sp:
        ds1, ds2 = _wf_bwd(dfs, t1, t2, ws, dens, ps)
        d1, d2 = d1 + dfs * ws, d2 + dfs * (dt(1.0) - ws)
    if ch:
        dc1, dc2 = _wf_bwd(dfc, t1, t2, wc, denc, pc)
        d1, d2 = d1 + dfc * wc, d2 + dfc * (dt(1.0) - wc)
    return out, (d1, d2, ds1, ds2, dc1, dc2)


def join_inputs(count, seed, dt=np.float32, eps=EPS32):
    """(t1, t2, s1, s2, c1, c2, g) of `count` elements in precision dt.  The maps look like 'nl' maps of non-negative features (map = feature + a
    positive attention term); the first PLANTED elements (as many as fit) put a + b of BOTH map pairs into the clamp's regimes: negative, zero,
    exactly eps, and one ulp above it.  Every planted sum is exact in dt (the last two by Sterbenz: b = eps - 2^-24), and the pairs are chosen so
    that neither 1 - w nor fs + fc cancels: each planted value is well conditioned and can be compared relative to its own size."""
    rng = np.random.default_rng(seed)
    t1, t2 = (rng.random(count) ** 2).astype(np.float32).astype(dt), (rng.random(count) ** 2).astype(np.float32).astype(dt)
    s1, s2, c1, c2 = ((t + rng.random(count) * 0.5).astype(np.float32).astype(dt) for t in (t1, t2, t1, t2))
    g = rng.standard_normal(count).astype(np.float32).astype(dt)
    eps = dt(eps)
    a = dt(2.0 ** -24)
    b, b2 = eps - a, np.nextafter(eps, dt(1.0)) - a
    assert a + b == eps and a + b2 == np.nextafter(eps, dt(1.0)) and a + b2 > eps
    plant_s = [(dt(-0.25), dt(0.125)), (dt(0.5), dt(-0.5)), (a, b), (a, b2)]
    plant_c = [(dt(0.125), dt(-0.25)), (dt(0.25), dt(-0.25)), (b, a), (b2, a)]
    for k in range(min(count, PLANTED)):
        (s1[k], s2[k]), (c1[k], c2[k]) = plant_s[k], plant_c[k]
    return t1, t2, s1, s2, c1, c2, g


def join_err(got, ref, planted):
    """(error of the ordinary elements relative to the largest of them, error of the planted clamp-regime elements each relative to its OWN size:
    their values are of order 1e7 t, and a bound scaled by them would hide everything else, one scaled by the rest would hide them)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    k = min(planted, ref.size)
    own = np.abs(got[:k] - ref[:k]) / np.maximum(np.abs(ref[:k]), 1e-30)
    own = np.where(ref[:k] == 0.0, np.where(got[:k] == 0.0, 0.0, np.inf), own)
    rest = float(np.abs(got[k:] - ref[k:]).max() / np.abs(ref[k:]).max()) if ref.size > k else 0.0
    return rest, float(own.max()) if k else 0.0
