"""Cases and a numpy float64 restatement of spatial_pooling(x, 'nl') (reference core/fusion.py:96-113) for golden F21.

The fixture tests/golden/f21_nonlocal.npz (written by tests/golden/make_golden_nonlocal.py from the reference's own code in float64)
holds results only; the inputs are rebuilt here from seeds.  Features are non-negative, like post-ReLU feature maps, and float32-exact,
so that the fp32 kernels and the float64 oracles start from the same numbers.  The gradient is that of sum(y * upstream(case)).

Arrays of more than SAMPLE_ABOVE elements are stored as a flat strided sample (sample_index) to keep the fixture small; the restatement
below is checked against those samples on the CPU and then serves as the full-tensor float64 reference of the GPU tests.
"""
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
