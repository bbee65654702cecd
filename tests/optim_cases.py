"""Cases and the fp64 definition of mmif_clip_adam_step (csrc/misc.hip: sumsq_kernel + adam_kernel): clip_grad_norm_(max_norm) + Adam on flat
fp32 buffers.  No GPU and no torch needed: tests/test_optim_oracle_cpu.py pins the definition to torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam in float64 and to oracle.fusion_oracle; tests/test_gpu_optim_sweep.py runs every case on the device.

Definition (every float the entry point takes enters with its fp32 value):
  norm = grad_scale ||g||_2;  coef = min(1, max_norm / (norm + 1e-6)), a NaN norm giving a NaN coefficient as torch's clamp does;
  max_norm <= 0: coef = 1;  g' = g coef grad_scale;  m += (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2;
  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps),  bc = 1 - b^step.
A +inf gradient gives norm = inf, coef = 0: the inf element becomes NaN (inf * 0), every other gradient counts as 0.

Bounds (u = 2^-24), derived from the kernel source.  The sum of squares is all-positive, so its error is relative: a thread's fma chain of
T = ceil(numel / (blocks 256)) terms, the block tree (6 shuffle steps + 4 waves), then in adam_kernel ceil(blocks / 256) partials per thread
and the same tree: Ks = T + 10 + ceil(blocks / 256) + 10 roundings.
  norm_rel = (Ks / 2 + 3) u                       sqrt halves the relative error; sqrtf (1 ulp = 2 u allowed), the product with grad_scale
  coef_rel = norm_rel + 3 u where coef < 1        the fp32 sum with 1e-6f, the quotient; coef = 1 exactly where the quotient is clearly
                                                   above 1 (every case is: test_optim_oracle_cpu.py asserts the distance)
  gi_rel   = coef_rel + 2 u                       coef grad_scale, g (coef grad_scale)
  mi_err   = (1 - b1) gi_err + 4 u (|m| + (1 - b1)(|gi| + |m|))
  vi_err   = 2 (1 - b2) |gi| gi_err + 5 u (b2 v + (1 - b2) gi^2)          all-positive: vi_rel = vi_err / vi
  den_rel  = vi_rel / 2 + 5 u                     sqrtf, fp32(1 / sqrt(bc2)), the product, + eps
  q_err    = mi_err / den + |mi / den| den_rel + u |mi / den|
  p_err    = step (q_err + 2 u |q|) + u |p'|      fp32(lr / bc1), the product, the difference; where the update is exactly 0 (zero
                                                   gradient on zero moments) p - 0 is exact: bound 0, the parameter comes back bit-identical
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
SENT = -1024.0
ADAM_PARTIALS = 1024
NUMELS = (1, 255, 256, 257, 262143, 262144, 262145, 3 * 262144 + 17)
STEPS = (1, 2, 1000)
GRAD_SCALES = (1.0, 0.5, 0.125)
CLIPS = ("off", "below", "above", "near_lo", "near_hi", "tiny")     # max_norm 0 | 5, norm << 5 | 5, norm >> 5 | norm = 5 (1 -+ 5e-4) | max_norm = norm = 1e-5
SPECIALS = ("zero", "stretch", "nan", "inf")
LR, B1, B2, ADAM_EPS = (float(np.float32(v)) for v in (1e-4, 0.9, 0.999, 1e-8))

MUTATIONS = ("no_1e6", "coef_uncapped", "grad_scale_not_in_norm", "bias_correction_step_minus_1", "eps_inside_root", "v_from_unclipped",
             "beta1_swapped", "nan_norm_dropped")


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@dataclass(frozen=True)
class Case:
    numel: int
    clip: str = "below"
    step: int = 1
    grad_scale: float = 1.0
    moments: bool = False     # non-zero incoming moments
    special: str = ""         # one of SPECIALS
    norm_out: bool = True     # False: NULL
    offset: bool = False      # buffers start at an odd float offset

    @property
    def id(self):
        return f"adam-{self.numel}-{self.clip}-step{self.step}-gs{self.grad_scale}" + ("-moments" if self.moments else "") + \
            (("-" + self.special) if self.special else "") + ("" if self.norm_out else "-nonormout") + ("-odd" if self.offset else "")

    @property
    def blocks(self):
        return min((self.numel + 255) // 256, ADAM_PARTIALS)

    @property
    def max_norm(self):
        return float(np.float32({"off": 0.0, "tiny": 1e-5}.get(self.clip, 5.0)))

    @property
    def target_norm(self):
        return {"off": 3.0, "below": 0.05, "above": 400.0, "near_lo": 5.0 * (1 - 5e-4), "near_hi": 5.0 * (1 + 5e-4), "tiny": 1e-5}[self.clip]

    def Ks(self):
        T = -(-self.numel // (self.blocks * 256))
        return T + 10 + -(-self.blocks // 256) + 10

    def mutations(self):
        if self.special == "nan":
            return ["nan_norm_dropped"] if self.max_norm > 0 else []
        if self.special:
            return []
        m = ["beta1_swapped"]
        # sqrt(v + eps) against sqrt(v) + eps shows where sqrt(v) is not far above sqrt(eps) = 1e-4: small clipped gradient elements
        if min(self.target_norm, self.max_norm or self.target_norm) / np.sqrt(self.numel) < 5e-3:
            m.append("eps_inside_root")
        if self.clip == "tiny":
            m.append("no_1e6")
        if self.clip in ("below", "near_lo"):
            m.append("coef_uncapped")
        if self.grad_scale != 1.0 and self.clip in ("above", "tiny", "near_hi"):
            m.append("grad_scale_not_in_norm")
        if self.step >= 2:
            m.append("bias_correction_step_minus_1")
        if self.clip in ("above", "tiny"):
            m.append("v_from_unclipped")
        return m


def _cases():
    cs = []
    for i, numel in enumerate(NUMELS):
        for j, clip in enumerate(CLIPS):
            cs.append(Case(numel, clip, STEPS[(i + j) % 3], GRAD_SCALES[(i + 2 * j) % 3], moments=bool((i + j) % 2) or clip == "tiny",
                           norm_out=(3 * i + j) % 7 != 6, offset=bool((i + j // 2) % 2)))
    for i, numel in enumerate((257, 262145, NUMELS[-1])):
        for j, sp in enumerate(SPECIALS):
            cs.append(Case(numel, "above" if sp in ("nan", "inf") else "below", STEPS[(i + j) % 3], GRAD_SCALES[(i + j) % 3], moments=(sp != "zero"),
                           special=sp, offset=bool((i + j) % 2)))
    cs.append(Case(257, "off", 2, 0.5, moments=True, special="nan"))       # clipping disabled: only the NaN element is poisoned
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"

_OPS = {}


def gradient(c: Case, rng):
    g = rng.standard_normal(c.numel)
    if c.special == "zero":
        return np.zeros(c.numel)
    if c.special == "stretch":
        g[stretch(c)] = 0.0
    # scaled so that grad_scale ||g|| is the target; the fp32 rounding moves the norm by a few u relative, far less than 5e-4
    return f32(g * (c.target_norm / (c.grad_scale * np.sqrt((g * g).sum()))))


def stretch(c):
    return slice(c.numel // 3, c.numel // 3 + max(c.numel // 4, 1))


def operands(c: Case) -> dict:
    if c.id in _OPS:
        return _OPS[c.id]
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    o = {"p": f32(rng.standard_normal(c.numel) * 0.1), "g": gradient(c, rng)}
    gmag = c.target_norm / c.grad_scale / np.sqrt(c.numel)
    if c.moments:
        o["m"], o["v"] = f32(rng.standard_normal(c.numel) * gmag * 0.5), f32(rng.uniform(0.1, 2.0, c.numel) * gmag ** 2)
    else:
        o["m"], o["v"] = np.zeros(c.numel), np.zeros(c.numel)
    if c.special == "stretch":
        o["m"][stretch(c)] = 0.0
        o["v"][stretch(c)] = 0.0
    if c.special in ("nan", "inf"):
        o["g"][c.numel // 2] = np.nan if c.special == "nan" else np.inf
    _OPS[c.id] = o
    while len(_OPS) > 3:
        _OPS.pop(next(iter(_OPS)))
    return o


def adam_on(p, g, m, v, step, max_norm, grad_scale, lr=LR, b1=B1, b2=B2, eps=ADAM_EPS, mut=None):
    """one step in float64: dict(p, m, v, norm, coef, quotient q of max_norm / (norm + 1e-6))"""
    with np.errstate(all="ignore"):
        norm = (1.0 if mut == "grad_scale_not_in_norm" else grad_scale) * np.sqrt((g * g).sum())
        q = max_norm / (norm + (0.0 if mut == "no_1e6" else 1e-6)) if max_norm > 0 else np.inf
        if max_norm <= 0:
            coef = 1.0
        elif mut == "coef_uncapped":
            coef = q
        elif mut == "nan_norm_dropped":
            coef = float(np.fmin(1.0, q))
        else:
            coef = float(np.minimum(1.0, q))          # propagates NaN
        gi = g * (coef * grad_scale)
        k1 = b1 if mut == "beta1_swapped" else 1.0 - b1
        mi = m + (gi - m) * k1
        gv = g * grad_scale if mut == "v_from_unclipped" else gi
        vi = b2 * v + (1.0 - b2) * gv * gv
        t = step - 1 if mut == "bias_correction_step_minus_1" else step
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        den = np.sqrt(vi / bc2 + eps) if mut == "eps_inside_root" else np.sqrt(vi) / np.sqrt(bc2) + eps
        upd = (lr / bc1) * (mi / den)
        return dict(p=p - upd, m=mi, v=vi, norm=norm, coef=coef, q=q, gi=gi, den=den, upd=upd, step_size=lr / bc1)


def bounds(c: Case, o, r, lr=LR, b1=B1, b2=B2):
    """per-output bounds of the true definition r = adam_on(...) (see the module docstring); NaN / inf wants carry bound 0"""
    with np.errstate(all="ignore"):
        norm_rel = (c.Ks() / 2 + 3) * U
        coef_rel = norm_rel + 3 * U if (c.max_norm > 0 and r["q"] < 1) else 0.0
        gi_rel = coef_rel + 2 * U
        gi, mi, vi = np.abs(r["gi"]), np.abs(r["m"]), r["v"]
        gi_err = gi * gi_rel
        mi_err = (1 - b1) * gi_err + 4 * U * (np.abs(o["m"]) + (1 - b1) * (gi + np.abs(o["m"])))
        vi_err = 2 * (1 - b2) * gi * gi_err + 5 * U * (b2 * o["v"] + (1 - b2) * gi * gi)
        vi_rel = np.where(vi > 0, vi_err / np.where(vi > 0, vi, 1.0), 0.0)
        den_rel = vi_rel / 2 + 5 * U
        qq = mi / r["den"]
        q_err = mi_err / r["den"] + qq * den_rel + U * qq
        p_err = r["step_size"] * (q_err + 2 * U * qq) + U * np.abs(r["p"])
        p_err = np.where(r["upd"] == 0, 0.0, p_err)
        norm_err = norm_rel * r["norm"]
    clean = lambda b, w: np.where(np.isfinite(w), b, 0.0)
    return dict(p=clean(p_err, r["p"]), m=clean(mi_err, r["m"]), v=clean(vi_err, r["v"]),
                norm=clean(np.asarray([norm_err]), np.asarray([r["norm"]])))


@dataclass
class Out:
    name: str
    want: np.ndarray
    bound: np.ndarray


def define_on(c: Case, o, mut=None):
    """the case's call on the operands o (p, g, m, v: float64 arrays holding fp32 values)"""
    true = adam_on(o["p"], o["g"], o["m"], o["v"], c.step, c.max_norm, c.grad_scale)
    r = true if mut is None else adam_on(o["p"], o["g"], o["m"], o["v"], c.step, c.max_norm, c.grad_scale, mut=mut)
    b = bounds(c, o, true)
    outs = [Out("params", r["p"], b["p"]), Out("exp_avg", r["m"], b["m"]), Out("exp_avg_sq", r["v"], b["v"])]
    if c.norm_out:
        outs.append(Out("norm_out", np.asarray([r["norm"]]), b["norm"]))
    return outs


def define(c: Case, mut=None):
    return define_on(c, operands(c), mut)


def propagate(E, r, b, b1=B1, b2=B2):
    """bounds of step k of a trajectory the device carries in fp32 against the float64 trajectory, to first order: E = the bounds after step
    k - 1 (None: the states agree), r = adam_on of the float64 trajectory at step k, b = its one-step bounds.  The gradients are the same on
    both sides, so m and v inherit b1 E_m and b2 E_v; the update step m / (sqrt(v) / sqrt(bc2) + eps) inherits
    step (b1 E_m / den + |m| / den^2 * b2 E_v / (2 sqrt(v) sqrt(bc2))), and p adds that to what it carried."""
    if E is None:
        return dict(b)
    with np.errstate(all="ignore"):
        em, ev = b1 * E["m"], b2 * E["v"]
        inv_bc2_sqrt = np.where(r["v"] > 0, (r["den"] - ADAM_EPS) / np.sqrt(np.where(r["v"] > 0, r["v"], 1.0)), 0.0)      # 1 / sqrt(bc2)
        dden = np.where(r["v"] > 0, ev / (2 * np.sqrt(np.where(r["v"] > 0, r["v"], 1.0))) * inv_bc2_sqrt, 0.0)
        dupd = r["step_size"] * (em / r["den"] + np.abs(r["m"]) / r["den"] ** 2 * dden)
    return dict(p=E["p"] + b["p"] + dupd, m=em + b["m"], v=ev + b["v"], norm=b["norm"])
