"""Cases and fp64 definitions for the fp32 NCHW norm + activation kernels of csrc/norm.hip: mmif_norm_act_fwd / _bwd (kind 0 BatchNorm2d in
training mode, 1 BatchNorm2d in eval mode, 2 GroupNorm(c, c); act 0 none, 1 ReLU, 2 LeakyReLU(slope), 3 Tanh, 4 ReLU6), the staged cross-rank
BatchNorm (mmif_bn_moments -> all-reduce -> mmif_bn_apply_fwd, mmif_bn_bwd_sums -> all-reduce -> mmif_bn_apply_bwd) and mmif_act_fwd / _bwd.
No GPU and no torch needed: tests/test_norm_oracle_cpu.py pins the definitions to torch's float64 autograd, to oracle.fusion_oracle and to
tests/golden/f13_n4_norm.npz, proves the table complete and able to tell every listed wrong definition from the true one;
tests/test_gpu_norm_sweep.py runs every case on the device.

Definitions (include/mmif.h is the contract).  Every scalar the entry point takes as a float (eps, momentum, slope) enters the definition
with its fp32 value.  Forward: two-pass float64 mean and biased variance over (N, H, W) (kind 0) or (H, W) per plane (kind 2), the running
buffers for kind 1; rstd = 1 / sqrt(var + eps); y = act(gamma (x - mean) rstd + beta); running = (1 - momentum) running + momentum batch with
the unbiased variance (m / (m - 1) left out at m = 1); stats = (mean, rstd).  m = 1 (torch refuses it): var = 0, y = act(beta), dx = 0.
Backward: takes the STORED fp32 x, y, gy, stats, gamma as given -- what the entry point receives: the activation derivative is decided from
the stored y, xhat = (x - stats.mean) stats.rstd in float64 -- so no near-tie between a kernel's and the definition's forward can flip a
derivative and every element of every case is compared.
The staged cases are two emulated ranks (1 + 2 samples): the definition is full-batch BatchNorm, each rank's chan_sums / dgamma / dbeta are
its local sums.

Bounds (u = 2^-24, e = 2^-53), derived from the kernel source, never fitted; selections (ReLU / ReLU6 / no activation in mmif_act_*) are
bit-exact.  L = ceil(hw / 256) + 6 + 4 + n + 4 counts the float64 additions that feed one statistic (a thread's strided partial, 6 shuffle
steps, 4 waves, n planes, the division / square / difference).
 forward   mean_err = u |mean| + L e mean|x|                      (the stored mean is rounded to fp32: dominates the ill-conditioned case;
                                                                   at m = 1 the mean is the fp32 element itself: no u |mean|)
           var_err  = 2 L e E[x^2]                                (one-pass variance s2 / m - mean^2: cancellation)
           rstd_err = rstd (u + var_err / (var + eps))            (fp32 store; kind 1: 4 u rstd for the fp32 add, sqrt, divide)
           xh_err   = (mean_err + u |x - mean|) rstd + |x - mean| rstd_err + u |xh|
           z_err    = |gamma| xh_err + u |gamma xh| + u (|gamma xh| + |beta|)
           y_err    = z_err (act 0, 1, 4: Lipschitz 1), max(1, slope) z_err + u |y| (act 2), z_err + TANH_ULP 2 u |y| (act 3)
           running  : 4 u (|1 - mom| |old| + |mom| |batch|) + |mom| (error of the batch value, + u |unbiased var|)
 backward  d_err  = u y^2 + u |d| (tanh: 1 - y y), else 0;  dz_err = |gy| d_err + u |dz| (acts 2, 3), 0 for selections
           xh_err = 2 u |xh| (the kernel's fp32 (x - mean) rstd against the float64 one on the same stored stats)
           S1 = sum dz, S2 = sum dz xh in float64: the summed element errors + L e sum |terms|;  dbeta, dgamma: + u |S| (fp32 store)
           a = fp32(S1 / m), b = fp32(S2 / m): u |a| + S1_err / m;  A = |dz| + |a| + |xh| |b|
           dx = fp32(gamma rstd) * fp32(dz - a - xh b):  |gamma| rstd (dz_err + a_err + xh_err |b| + |xh| b_err + 5 u A)
           eval: |gamma| rstd (dz_err + 2 u |dz|)
 tanhf     no published accuracy figure for the device's tanhf ships with the ROCm installation this suite runs on, so the platform's tanh
           was measured: torch.tanh (float32, on the device) against float64 tanh over z in [-12, 12] (2^22 points, wider and denser than
           the cases' z range needs) has a maximum error of 1.405 ulp on an MI355X (TANH_ULP_MEASURED = 1.41).  That measures the
           platform's implementation, not this project's kernel; twice the figure is allowed, since the two may differ in implementation:
           TANH_ULP = 2 TANH_ULP_MEASURED = 2.82.  tests/test_gpu_norm_sweep.py measures the figure again on every run and fails if the
           platform's tanh has become worse than recorded.
The grid-stride loops of the apply kernels cap at 65 535 * 16 blocks (grid1d_n): a second trip needs about 2.7e8 elements, over 1 GiB per
tensor.  That is out of scope here; no case pretends to reach it.  What the cases do reach: planes past 256 elements (a second trip and a
ragged tail of the block-strided moment loops) and c > 256 (a second block of the 256-thread finish kernels).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
E64 = 2.0 ** -53
SENT = -1024.0
TANH_ULP_MEASURED = 1.41       # max ulp error of the device's float32 tanh against float64: 1.405 measured on an MI355X (see the docstring)
TANH_ULP = 2.0 * TANH_ULP_MEASURED
ACTS = ("none", "relu", "leaky", "tanh", "relu6")
EPS = ("norm_fwd", "norm_bwd", "staged_fwd", "staged_bwd", "act_fwd", "act_bwd")
HW = {1: (1, 1), 2: (1, 2), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (1, 257), 511: (7, 73), 513: (27, 19),
      1000: (25, 40)}
CHANNELS = (1, 3, 256, 257)
COUNTS = (0, 1, 255, 256, 257, 1000)
MOMENTA = (0.1, 1.0, 0.0)
EPSILONS = (1e-5, 1e-3)
SLOPES = (0.2, 0.01)
RANKS = (1, 2)                 # the staged cases split n = 3 unevenly

MUTATIONS = ("biased_running_var", "momentum_swapped", "eps_outside_root", "gn_stats_per_channel", "bn_stats_per_plane", "bwd_m_is_hw",
             "staged_local_count", "no_xhat_term", "train_formula_in_eval", "dgamma_dbeta_swapped", "null_gamma_is_zero", "relu_ge_zero",
             "relu6_le_six", "leaky_slope_on_positive", "tanh_one_minus_y")


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@dataclass(frozen=True)
class Case:
    ep: str                   # one of EPS
    kind: int = 0
    act: int = 0
    n: int = 1
    c: int = 1
    hw: int = 1
    gamma: bool = True        # False: NULL
    beta: bool = True
    dgamma: bool = True
    dbeta: bool = True
    running: bool = True      # kind 0 forward: running buffers given
    momentum: float = 0.1
    eps: float = 1e-5
    slope: float = 0.2
    plant: str = ""           # const | ties | illcond
    offset: bool = False      # operands start at an odd float offset
    count: int = 0            # mmif_act_*

    @property
    def id(self):
        if self.ep.startswith("act"):
            return f"{self.ep}-{ACTS[self.act]}-{self.count}-s{self.slope}" + ("-ties" if self.plant else "") + ("-odd" if self.offset else "")
        s = f"{self.ep}-k{self.kind}-{ACTS[self.act]}-{self.n}x{self.c}x{self.hw}-mom{self.momentum}-eps{self.eps}-s{self.slope}"
        for flag, name in ((self.gamma, "nogamma"), (self.beta, "nobeta"), (self.dgamma, "nodgamma"), (self.dbeta, "nodbeta"), (self.running, "norunning")):
            if not flag:
                s += "-" + name
        return s + (("-" + self.plant) if self.plant else "") + ("-odd" if self.offset else "")

    @property
    def shape(self):
        return (self.n, self.c) + HW[self.hw]

    @property
    def m(self):
        return self.hw if self.kind == 2 else self.n * self.hw

    @property
    def fwd(self):
        return self.ep in ("norm_fwd", "staged_fwd", "act_fwd")

    def scalars(self):
        """(eps, momentum, slope) as the entry point receives them"""
        return tuple(float(np.float32(v)) for v in (self.eps, self.momentum, self.slope))

    def mutations(self):
        """the wrong definitions that can show on this case"""
        if self.plant == "illcond":
            return []
        m = []
        norm, bwd = not self.ep.startswith("act"), not self.fwd
        if norm and self.fwd and self.kind == 0 and self.running and self.m > 1:
            if self.momentum > 0:
                m.append("biased_running_var")
            m.append("momentum_swapped")
        if norm and self.kind != 1 and self.fwd and self.m > 1 and self.plant != "const":
            m.append("eps_outside_root")
        if self.ep == "norm_fwd" and self.kind == 2 and self.n > 1 and self.hw > 1:
            m.append("gn_stats_per_channel")
        if self.ep in ("norm_fwd", "staged_fwd") and self.kind == 0 and self.n > 1 and self.hw > 1:
            m.append("bn_stats_per_plane")
        if self.ep == "norm_bwd" and self.kind == 0 and self.n > 1:
            m.append("bwd_m_is_hw")
        if self.ep == "staged_bwd":
            m.append("staged_local_count")
        if norm and bwd and self.kind != 1 and self.m > 1:
            m.append("no_xhat_term")
        if self.ep == "norm_bwd" and self.kind == 1:
            m.append("train_formula_in_eval")
        if norm and bwd and self.dgamma and self.dbeta:
            m.append("dgamma_dbeta_swapped")
        if norm and not self.gamma:
            m.append("null_gamma_is_zero")
        if bwd and self.plant == "ties":
            m += {1: ["relu_ge_zero"], 4: ["relu6_le_six"]}.get(self.act, [])
        if self.act == 2 and (self.count > 0 or norm):
            m.append("leaky_slope_on_positive")
        if bwd and self.act == 3 and (self.count > 0 or norm):
            m.append("tanh_one_minus_y")
        return m


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
def _cases():
    cs = []
    hws = list(HW)
    i = 0
    # ---- kind x act x direction, every plane size, channel count, n, momentum, eps, slope in rotation
    for ep in ("norm_fwd", "norm_bwd"):
        for kind in (0, 1, 2):
            for act in range(5):
                hw = hws[(7 * i + 3) % len(hws)]
                c = CHANNELS[i % 4]
                if c >= 256 and hw > 65:
                    c = 3
                cs.append(Case(ep, kind, act, n=(1, 2, 3)[(i + i // 3) % 3], c=c, hw=hw, momentum=MOMENTA[i % 3], eps=EPSILONS[i % 2],
                               slope=SLOPES[(i // 2) % 2], offset=bool(i % 2), plant="ties" if (ep == "norm_bwd" and act and hw >= 63) else ""))
                i += 1
    # ---- the plane sizes the rotation leaves out for a direction, and c = 256 / 257 in both
    for ep in ("norm_fwd", "norm_bwd"):
        have = {c.hw for c in cs if c.ep == ep}
        for j, hw in enumerate(h for h in hws if h not in have):
            cs.append(Case(ep, (0, 2)[j % 2], (j + 1) % 5, n=2, c=3, hw=hw, eps=EPSILONS[j % 2]))
        for j, (c, hw, n) in enumerate(((256, 64, 2), (257, 2, 3), (257, 65, 1), (256, 1, 2))):
            cs.append(Case(ep, (0, 2, 1, 0)[j], (1, 3, 2, 4)[j], n=n, c=c, hw=hw, offset=bool(j % 2), plant="ties" if ep == "norm_bwd" and hw >= 63 else ""))
    # ---- NULL operands
    for kind in (0, 1, 2):
        for g, b in ((False, False), (False, True), (True, False)):
            cs.append(Case("norm_fwd", kind, (1, 2, 3)[kind], n=2, c=3, hw=65, gamma=g, beta=b, offset=not g))
        for g, dg, db in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            cs.append(Case("norm_bwd", kind, (2, 3, 1)[kind], n=2, c=3, hw=65, gamma=g, dgamma=dg, dbeta=db, offset=dg))
    for mom in MOMENTA:
        cs.append(Case("norm_fwd", 0, 1, n=2, c=3, hw=257, running=False, momentum=mom))
        cs.append(Case("norm_fwd", 0, 0, n=3, c=3, hw=63, momentum=mom, eps=1e-3))
    # ---- planted values
    for kind in (0, 2):
        for eps in EPSILONS:
            cs.append(Case("norm_fwd", kind, 2, n=2, c=3, hw=257, eps=eps, plant="const"))
            cs.append(Case("norm_bwd", kind, 0, n=2, c=3, hw=257, eps=eps, plant="const"))
    for kind in (0, 1, 2):
        for act in (1, 2, 3, 4):
            cs.append(Case("norm_bwd", kind, act, n=2, c=3, hw=255, plant="ties", slope=SLOPES[act % 2]))
    cs.append(Case("norm_fwd", 0, 0, n=2, c=3, hw=513, plant="illcond"))
    cs.append(Case("norm_fwd", 2, 3, n=2, c=3, hw=256, plant="illcond"))
    for ep in ("norm_fwd", "norm_bwd"):          # m = 1
        cs.append(Case(ep, 0, 1, n=1, c=3, hw=1, momentum=0.1))
        cs.append(Case(ep, 2, 3, n=2, c=3, hw=1))
    # ---- staged BatchNorm: two ranks, 1 + 2 samples
    for j, act in enumerate(range(5)):
        hw, c = (63, 257, 1000, 2, 513)[j], (257, 3, 1, 256, 3)[j]
        cs.append(Case("staged_fwd", 0, act, n=3, c=c, hw=hw, momentum=MOMENTA[j % 3], eps=EPSILONS[j % 2], slope=SLOPES[j % 2], offset=bool(j % 2)))
        cs.append(Case("staged_bwd", 0, act, n=3, c=c, hw=hw, slope=SLOPES[j % 2], offset=not j % 2, plant="ties" if act and hw >= 63 else ""))
    cs.append(Case("staged_fwd", 0, 1, n=3, c=3, hw=65, gamma=False, beta=False, running=False))
    cs.append(Case("staged_bwd", 0, 2, n=3, c=3, hw=65, gamma=False, dgamma=False, dbeta=False))
    cs.append(Case("staged_bwd", 0, 4, n=3, c=3, hw=255, dgamma=False, plant="ties"))
    # ---- the activation alone
    for ep in ("act_fwd", "act_bwd"):
        for act in range(5):
            for j, count in enumerate(COUNTS):
                cs.append(Case(ep, act=act, count=count, slope=SLOPES[(act + j) % 2], offset=bool((act + j) % 2),
                               plant="ties" if ep == "act_bwd" and act and count >= 255 else ""))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------------------------------------------------------------------
# definitions
# ------------------------------------------------------------------------------------------------------------------------------
def act_fwd(z, act, slope, mut=None):
    if act == 1:
        return np.maximum(z, 0.0)
    if act == 2:
        if mut == "leaky_slope_on_positive":
            return np.where(z > 0, z * slope, z)
        return np.where(z > 0, z, z * slope)
    if act == 3:
        return np.tanh(z)
    if act == 4:
        return np.minimum(np.maximum(z, 0.0), 6.0)
    return z + 0.0


def act_dydz(y, act, slope, mut=None):
    """every derivative is a function of the output y"""
    one = np.ones_like(y)
    if act == 1:
        return np.where((y >= 0) if mut == "relu_ge_zero" else (y > 0), 1.0, 0.0)
    if act == 2:
        return np.where(y > 0, slope, 1.0) if mut == "leaky_slope_on_positive" else np.where(y > 0, 1.0, slope)
    if act == 3:
        return 1.0 - y if mut == "tanh_one_minus_y" else 1.0 - y * y
    if act == 4:
        return np.where((y > 0) & ((y <= 6) if mut == "relu6_le_six" else (y < 6)), 1.0, 0.0)
    return one


def _axes(kind, mut=None):
    per_plane = (kind == 2) != (mut in ("gn_stats_per_channel", "bn_stats_per_plane"))
    return (2, 3) if per_plane else (0, 2, 3)


def _bc(v, c):
    """a per-channel vector (or None -> the neutral value is the caller's) as [1, c, 1, 1]"""
    return np.asarray(v, np.float64).reshape(1, c, 1, 1)


def fwd_on(x, gamma, beta, kind, act, eps, slope, running=None, momentum=0.1, mut=None):
    """float64 forward on float64 arrays: dict(y, mean, rstd [n or 1, c, 1, 1], var, running_mean, running_var)"""
    n, c = x.shape[:2]
    if kind == 1:
        mean, var = _bc(running[0], c), _bc(running[1], c)
    else:
        ax = _axes(kind, mut)
        mean = x.mean(ax, keepdims=True)
        var = ((x - mean) ** 2).mean(ax, keepdims=True)
    rstd = 1.0 / (np.sqrt(var) + eps) if mut == "eps_outside_root" else 1.0 / np.sqrt(var + eps)
    g = (0.0 if mut == "null_gamma_is_zero" else 1.0) if gamma is None else _bc(gamma, c)
    b = 0.0 if beta is None else _bc(beta, c)
    xh = (x - mean) * rstd
    out = dict(y=act_fwd(g * xh + b, act, slope, mut), mean=mean, rstd=rstd, var=var, xh=xh)
    if kind == 0 and running is not None:
        m = x.shape[0] * x.shape[2] * x.shape[3]
        bm, bv = x.mean((0, 2, 3)), x.var((0, 2, 3))        # (the per-plane mutation leaves the running update alone)
        unb = bv if (m == 1 or mut == "biased_running_var") else bv * m / (m - 1)
        wo, wn = (momentum, 1.0 - momentum) if mut == "momentum_swapped" else (1.0 - momentum, momentum)
        out["running_mean"], out["running_var"] = wo * running[0] + wn * bm, wo * running[1] + wn * unb
    return out


def bwd_on(x, y, gy, mean, rstd, gamma, kind, act, slope, m=None, mut=None):
    """float64 backward from the arrays as given (mean, rstd broadcastable [n or 1, c, 1, 1]): dict(dx, dgamma, dbeta, S1, S2 per statistic)"""
    n, c = x.shape[:2]
    dz = gy * act_dydz(y, act, slope, mut)
    xh = (x - mean) * rstd
    g = (0.0 if mut == "null_gamma_is_zero" else 1.0) if gamma is None else _bc(gamma, c)
    s1, s2 = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    out = dict(dbeta=s2 if mut == "dgamma_dbeta_swapped" else s1, dgamma=s1 if mut == "dgamma_dbeta_swapped" else s2, dz=dz, xh=xh)
    if kind == 1 and mut != "train_formula_in_eval":
        out["dx"] = g * rstd * dz
        return out
    ax = (2, 3) if kind == 2 else (0, 2, 3)
    if m is None:
        m = x.shape[2] * x.shape[3] * (1 if (kind == 2 or mut == "bwd_m_is_hw") else n)
    S1, S2 = dz.sum(ax, keepdims=True), (dz * xh).sum(ax, keepdims=True)
    out["S1"], out["S2"], out["m"] = S1, S2, m
    out["dx"] = g * rstd * (dz - S1 / m - (0.0 if mut == "no_xhat_term" else xh * (S2 / m)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
TIES = {1: (0.0, -0.0), 2: (0.0, -0.0), 3: (1.0, -1.0), 4: (0.0, -0.0, 6.0)}
_OPS = {}


def _plant(rng, y, gy, act):
    """exact ties in the stored y, each with a clearly non-zero incoming gradient"""
    flat, gflat = y.reshape(-1), gy.reshape(-1)
    k = min(flat.size // 4, 24)
    idx = rng.choice(flat.size, size=k, replace=False)
    for j, i in enumerate(idx):
        flat[i] = TIES[act][j % len(TIES[act])]
        gflat[i] = f32(np.sign(gflat[i] + 1e-30) * (0.5 + abs(gflat[i])))


def tie_counts(y, act):
    return {repr(v): int(((y == v) & (np.signbit(y) == np.signbit(v))).sum()) for v in TIES.get(act, ())}


def operands(c: Case) -> dict:
    if c.id in _OPS:
        return _OPS[c.id]
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    eps, mom, slope = c.scalars()
    o = {}
    if c.ep.startswith("act"):
        x = f32(rng.standard_normal(c.count) * (4.0 if c.act == 4 else 1.5))
        o["x"] = x
        if c.ep == "act_bwd":
            o["y"], o["gy"] = f32(act_fwd(x, c.act, slope)), f32(rng.standard_normal(c.count))
            if c.plant == "ties":
                _plant(rng, o["y"], o["gy"], c.act)
    else:
        sig, mu = rng.uniform(0.5, 2.0, c.c), rng.standard_normal(c.c)
        if c.plant == "illcond":
            mu = 1000.0 * sig * np.where(rng.random(c.c) < 0.5, -1.0, 1.0)        # |mean| = 10^3 sigma
        x = f32(_bc(mu, c.c) + _bc(sig, c.c) * rng.standard_normal(c.shape))
        if c.plant == "const":
            v = f32(1.7)
            if c.kind == 2:
                x[0, 1] = v          # one plane
            else:
                x[:, 1] = v          # a whole channel
        o["x"] = x
        gs = 3.0 if c.act == 4 else 1.0
        o["gamma"] = f32(gs * (1.0 + 0.3 * rng.standard_normal(c.c)) * np.where(rng.random(c.c) < 0.3, -1.0, 1.0)) if c.gamma else None
        o["beta"] = f32(0.4 * rng.standard_normal(c.c) + (1.0 if c.act == 4 else 0.0)) if c.beta else None
        o["running"] = (f32(mu + 0.3 * rng.standard_normal(c.c)), f32(sig ** 2 * rng.uniform(0.7, 1.4, c.c))) if (c.running or c.kind == 1) else None
        if not c.fwd:
            f = fwd_on(x, o["gamma"], o["beta"], c.kind, c.act, eps, slope, o["running"], mom)
            o["y"], o["gy"] = f32(f["y"]), f32(rng.standard_normal(c.shape))
            shape = (c.n, c.c, 1, 1) if c.kind == 2 else (1, c.c, 1, 1)
            o["mean"], o["rstd"] = f32(np.broadcast_to(f["mean"], shape)), f32(np.broadcast_to(f["rstd"], shape))
            if c.plant == "ties":
                _plant(rng, o["y"], o["gy"], c.act)
    _OPS[c.id] = o
    while len(_OPS) > 8:
        _OPS.pop(next(iter(_OPS)))
    return o


def gn_given_running(c: Case):
    """kind 2 ignores the running buffers (include/mmif.h): the odd-offset forward cases hand them over all the same, as inputs that must come
    back untouched; the others pass NULL"""
    return c.ep == "norm_fwd" and c.kind == 2 and c.offset


def stats_array(mean, rstd):
    """[planes, 2] float64 = (mean, rstd) as the stats buffer holds them"""
    return np.stack([np.asarray(mean, np.float64).reshape(-1), np.asarray(rstd, np.float64).reshape(-1)], 1)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------
def L64(c):
    return -(-c.hw // 256) + 6 + 4 + c.n + 4


def act_err(z_err, y, act, slope):
    if act == 2:
        return max(1.0, abs(slope)) * z_err + U * np.abs(y)
    if act == 3:
        return z_err + TANH_ULP * 2 * U * np.abs(y)
    return z_err


def fwd_bounds(c, x, gamma, beta, f, running, eps, mom, slope):
    L = L64(c)
    ax = (2, 3) if c.kind == 2 else (0, 2, 3)
    mean, rstd, var = f["mean"], f["rstd"], f["var"]
    b = {}
    if c.kind == 1:
        mean_err, rstd_err, var_err = 0.0 * mean, 4 * U * rstd, 0.0
    else:
        # (m = 1: the mean is the fp32 element itself, its fp32 store is exact)
        mean_err = (U if c.m > 1 else 0.0) * np.abs(mean) + L * E64 * np.abs(x).mean(ax, keepdims=True)
        var_err = 2 * L * E64 * (x * x).mean(ax, keepdims=True)
        rstd_err = rstd * (U + var_err / (var + eps))
    g = 1.0 if gamma is None else np.abs(_bc(gamma, c.c))
    bt = 0.0 if beta is None else np.abs(_bc(beta, c.c))
    d, xh = np.abs(x - mean), np.abs(f["xh"])
    xh_err = (mean_err + U * d) * rstd + d * rstd_err + U * xh
    z_err = g * xh_err + U * g * xh + U * (g * xh + bt)
    b["y"] = act_err(z_err, f["y"], c.act, slope)
    b["stats"] = stats_array(np.broadcast_to(mean_err, mean.shape), np.broadcast_to(rstd_err, rstd.shape))
    if "running_mean" in f:
        m = c.m
        unb = var.reshape(-1) * (m / (m - 1) if m > 1 else 1.0)
        b["running_mean"] = 4 * U * (abs(1 - mom) * np.abs(running[0]) + mom * np.abs(mean.reshape(-1))) + mom * mean_err.reshape(-1)
        b["running_var"] = 4 * U * (abs(1 - mom) * np.abs(running[1]) + mom * unb) + \
            mom * (np.asarray(var_err).reshape(-1) * (m / (m - 1) if m > 1 else 1.0) + U * unb)
    return b


def dz_err_of(y, gy, dz, act):
    if act == 3:
        return np.abs(gy) * (U * y * y + U * np.abs(1 - y * y)) + U * np.abs(dz)
    if act == 2:
        return U * np.abs(dz)
    return 0.0 * dz


def bwd_bounds(c, gamma, y, gy, rstd, r, m):
    """r = bwd_on(...) of the true definition on the full batch; m: the count dx is formed with"""
    L = L64(c) + 1
    dz, xh = np.abs(r["dz"]), np.abs(r["xh"])
    dz_err = dz_err_of(y, gy, r["dz"], c.act)
    xh_err = 2 * U * xh
    t2_err = dz_err * xh + dz * xh_err
    g = 1.0 if gamma is None else np.abs(_bc(gamma, c.c))
    b = {}
    ch = (0, 2, 3)
    b["dbeta"] = U * np.abs(r["dbeta"]) + dz_err.sum(ch) + L * E64 * dz.sum(ch)
    b["dgamma"] = U * np.abs(r["dgamma"]) + t2_err.sum(ch) + L * E64 * (dz * xh).sum(ch)
    if "S1" not in r:
        b["dx"] = g * rstd * (dz_err + 2 * U * dz)
        return b
    ax = (2, 3) if c.kind == 2 else (0, 2, 3)
    S1_err = dz_err.sum(ax, keepdims=True) + L * E64 * dz.sum(ax, keepdims=True)
    S2_err = t2_err.sum(ax, keepdims=True) + L * E64 * (dz * xh).sum(ax, keepdims=True)
    a, bb = np.abs(r["S1"]) / m, np.abs(r["S2"]) / m
    a_err, b_err = U * a + S1_err / m, U * bb + S2_err / m
    A = dz + a + xh * bb
    b["dx"] = g * rstd * (dz_err + a_err + xh_err * bb + xh * b_err + 5 * U * A)
    b["S1"], b["S2"] = S1_err, S2_err
    return b


def dx_scale(c, gamma, rstd, r):
    g = 1.0 if gamma is None else np.abs(_bc(gamma, c.c))
    return float(np.max(g * rstd * np.abs(r["dz"])))


@dataclass
class Out:
    name: str
    want: np.ndarray          # float64; SENT where the call leaves the buffer alone
    bound: np.ndarray
    exact: bool = False       # a selection: compared bit for bit
    scale: float = 0.0        # magnitude of the terms the output is formed from, where that exceeds max |want| (dx: |gamma| rstd |dz|)


def _rank_slices():
    lo = 0
    for r, k in enumerate(RANKS):
        yield r, slice(lo, lo + k)
        lo += k


def define(c: Case, mut=None, o=None):
    """[Out] of everything the case's calls write (o: other stored operands than the case's own, for the chained checks)"""
    o = operands(c) if o is None else o
    eps, mom, slope = c.scalars()
    if c.ep == "act_fwd":
        y = act_fwd(o["x"], c.act, slope, mut)
        exact = c.act in (0, 1, 4)
        return [Out("y", y, np.zeros(y.shape) if exact else act_err(0.0 * y, y, c.act, slope), exact)]
    if c.ep == "act_bwd":
        dx = o["gy"] * act_dydz(o["y"], c.act, slope, mut)
        exact = c.act in (0, 1, 4)
        return [Out("dx", dx, np.zeros(dx.shape) if exact else dz_err_of(o["y"], o["gy"], dx, c.act), exact)]
    x, gamma, beta = o["x"], o["gamma"], o["beta"]
    if c.fwd:
        true = fwd_on(x, gamma, beta, c.kind, c.act, eps, slope, o["running"], mom)
        f = true if mut is None else fwd_on(x, gamma, beta, c.kind, c.act, eps, slope, o["running"], mom, mut)
        b = fwd_bounds(c, x, gamma, beta, true, o["running"], eps, mom, slope)
        planes = (c.n if c.kind == 2 else 1) * c.c
        full = lambda a: np.broadcast_to(a, (c.n, c.c, 1, 1))[:(c.n if c.kind == 2 else 1)]
        stats = stats_array(full(f["mean"]), full(f["rstd"]))
        assert stats.shape == (planes, 2) == b["stats"].shape
        outs = [("y", f["y"], b["y"]), ("stats", stats, b["stats"])]
        if "running_mean" in f:
            outs += [("running_mean", f["running_mean"], b["running_mean"]), ("running_var", f["running_var"], b["running_var"])]
        if c.ep == "norm_fwd":
            return [Out(*t) for t in outs]
        res = []
        L = L64(c)
        for r, sl in _rank_slices():
            xs = x[sl]
            s1, s2 = xs.sum((0, 2, 3)), (xs * xs).sum((0, 2, 3))
            cnt = float(xs.shape[0] * c.hw)
            chan = np.concatenate([np.stack([s1, s2], 1).reshape(-1), [cnt]])
            cb = np.concatenate([np.stack([L * E64 * np.abs(xs).sum((0, 2, 3)), L * E64 * s2], 1).reshape(-1), [0.0]])
            res.append(Out(f"chan_sums_r{r}", chan, cb))
            for name, want, bound in outs:
                res.append(Out(f"{name}_r{r}", want[sl] if name == "y" else want, bound[sl] if name == "y" else bound))
        return res
    y, gy, mean, rstd = o["y"], o["gy"], o["mean"], o["rstd"]
    true = bwd_on(x, y, gy, mean, rstd, gamma, c.kind, c.act, slope)
    b = bwd_bounds(c, gamma, y, gy, rstd, true, true.get("m", 1))
    if c.ep == "norm_bwd":
        r = true if mut is None else bwd_on(x, y, gy, mean, rstd, gamma, c.kind, c.act, slope, mut=mut)
        outs = [Out("dx", r["dx"], np.broadcast_to(b["dx"], r["dx"].shape), scale=dx_scale(c, gamma, rstd, true))]
        if c.dgamma:
            outs.append(Out("dgamma", r["dgamma"], b["dgamma"]))
        if c.dbeta:
            outs.append(Out("dbeta", r["dbeta"], b["dbeta"]))
        return outs
    res = []
    full = true if mut in (None, "staged_local_count") else bwd_on(x, y, gy, mean, rstd, gamma, 0, c.act, slope, mut=mut)
    for r, sl in _rank_slices():
        loc = bwd_on(x[sl], y[sl], gy[sl], mean, rstd, gamma, 0, c.act, slope, mut=None if mut == "staged_local_count" else mut)
        lb = bwd_bounds(c, gamma, y[sl], gy[sl], rstd, bwd_on(x[sl], y[sl], gy[sl], mean, rstd, gamma, 0, c.act, slope), 1)
        sums = np.stack([loc["S1"].reshape(-1), loc["S2"].reshape(-1)], 1).reshape(-1)
        res.append(Out(f"chan_sums_r{r}", sums, np.stack([lb["S1"].reshape(-1), lb["S2"].reshape(-1)], 1).reshape(-1)))
        if c.dgamma:
            res.append(Out(f"dgamma_r{r}", loc["dgamma"], lb["dgamma"]))
        if c.dbeta:
            res.append(Out(f"dbeta_r{r}", loc["dbeta"], lb["dbeta"]))
        dx = loc["dx"] if mut == "staged_local_count" else full["dx"][sl]
        res.append(Out(f"dx_r{r}", dx, np.broadcast_to(b["dx"], full["dx"].shape)[sl], scale=dx_scale(c, gamma, rstd, true)))
    return res
