"""Cases and fp64 definitions for the plain-NCHW fp32 "row n4" kernels: csrc/conv_general.hip (mmif_gconv_fwd / _dgrad / _wgrad,
mmif_gconvt_fwd / _dgrad / _wgrad, mmif_relu_bwd, mmif_channel_sum, mmif_dwconv_fwd / _dgrad / _wgrad, mmif_patchconv_fwd / _dgrad / _wgrad and
their workspace queries) and csrc/resample.hip (mmif_bilinear_up_fwd / _bwd, mmif_maxpool_nchw_fwd / _bwd, mmif_nearest_up_fwd / _bwd,
mmif_reflect_pad_fwd / _bwd).  numpy only: tests/test_general_oracle_cpu.py pins the definitions to torch's float64 operators, to
oracle.fusion_oracle and to the recorded reference arrays, proves the table complete and able to tell every listed wrong definition from the
true one; tests/test_gpu_general_sweep.py runs every case on the device.

Definitions (include/mmif.h is the contract; float64 on the stored fp32 operands; gradients take gy as given, already masked).
 conv        y[o][oy][ox] = b[o] + sum W[o][c][u][v] Xpad[c][oy s + u][ox s + v], extent floor((h + 2p - k) / s) + 1, ReflectionPad2d(p) or zeros
 dgrad       scatter of gy W onto the padded domain, then the padding's adjoint (every reflect image summed, or the crop)
 wgrad       dW[o][c][u][v] = sum gy[o][oy][ox] Xpad[c][oy s + u][ox s + v], db[o] = sum gy over the output extent
 convT       y[co][iy s - p + u][ix s - p + v] += x[ci][iy][ix] W[ci][co][u][v], extent (h - 1) s - 2p + k + output_padding; its gradients are
             written as the adjoints of that scatter (not through gconv_fwd); the "db" of mmif_gconvt_wgrad is the per-channel sum of x
 depth-wise  groups == channels, stride 1, padding k / 2;  patch conv: kernel == stride == s, padding 0, the rows and columns past
             floor(h / s) s are not read and get a gradient of exactly +0.0
 bilinear    align_corners=True: r = fp32(fp32(h - 1) / fp32(H - 1)), s = fp32(r Y), y0 = min((int) s, h - 1), y1 = min(y0 + 1, h - 1), l = fp32(s - y0)
             (ATen's area_pixel_compute_source_index, oracle.fusion_oracle._bilinear_weights); the backward is the transpose of that map
 selections  (bit-exact, exact=True: the fp32 bits, -0.0 is not +0.0) mmif_relu_bwd (g where y > 0, else +0.0); max-pool value, uint8 index of the
             FIRST maximum in row-major window order, the first NaN of a window wins, the routing of the gradient; nearest forward; reflect pad
             forward; the +0.0 remainder of patchconv_dgrad and maxpool_nchw_bwd.

Bounds (u = 2^-24), derived from the kernel source (csrc/conv_general.hip, csrc/resample.hip; the lines are named), never fitted.  A chain of
T fp32 FMAs or additions has an error of at most T u / (1 - T u) <= (T + 1) u times the sum A of the terms' magnitudes (T (T + 1) u <= 1 holds
to T = 4095; no chain here is longer); terms that are exactly 0 (tile overhang, channels past cin) add no error but are counted, as the kernel
runs them.  A is the same definition evaluated on the operands' magnitudes.
 gconv_fwd        T = cin k k (the c0 / cc / u / v loops, :52-77) + 1 (bias add :85); the ReLU is a 1-Lipschitz selection       (T + 2) u A
 gconv_dgrad      T = cout ceil(k / s)^2 (the taps that pass the divisibility test :124-131) + 1; with the reflect fold up to 9 images
                  are added one by one (:170-172)                                                                              (T + 2 [+ 9]) u A
 gconvt_fwd       the same gather with cin channels, + 1 for the bias                                                          (T + 2) u A
 gconvt_dgrad     = gconv_fwd's chain with cout channels, no bias                                                              (T + 1) u A
 gconv_wgrad      per thread 256 pixels per tile (:226) times trips = ceil(tiles / G) of the tile loop (:201), then G partials (:268);
                  G = min(max(1024 / (ceil(cin / 8) ceil(cout / 8)), 1), tiles) (wg_groups :484)                                (256 trips + G + 1) u A
                  db: 256 per tile (:223), + trips (:224), + G                                                                 (256 + trips + G + 1) u A
 channel_sum      n ceil(hw / 256) per thread (:284-287) + 6 shuffle steps + 4 waves (block_sum)                               (T + 11) u A
 dwconv_fwd       k k FMAs onto the bias (:303-305)                                                                            (k k + 1) u A
 dwconv_dgrad     k k taps for each of up to 9 images in one chain (:329-339)                                                  (9 k k + 1) u A
 dwconv_wgrad     n ceil(hw / 256) per thread (:353-361) + 6 + 4                                                               (T + 11) u A
 patchconv_fwd    ceil(s s / L) FMAs per lane (:392), log2 L butterfly steps (:397), the bias (:398)                            (T + 2) u A
 patchconv_dgrad  one product                                                                                                  u |dx|
 patchconv_wgrad  a lane takes every lanes-th of the chunk's per ow outputs (:428; lanes = 256 / (s s), per = ceil(n (h / s) / 64)), the lanes are
                  added (:442), then the 64 chunks (:458)                                                                      (ceil(per ow / lanes) + lanes + 64 + 1) u A
 bilinear fwd     each term passes the roundings of 1 - l (twice), two products, the inner and the outer sum: 6               7 u A
                  + per axis (u (s + l)) |x[y1] - x[y0]| (interpolated along the other axis): a compiler that contracts l = s - y0 into
                  fma(r, Y, -y0) skips the rounding of s (<= u s) and rounds the result instead (<= u l); s - y0 itself is exact
 bilinear bwd     the row chain has as many terms as output columns map to ix, the outer one as many as rows map to iy (:56-65), 3 for
                  the weights and products                                                                                     (Tx + Ty + 4) u A
                  + the same contraction term through the transposed map
 nearest bwd      s s additions (:153-154)                                                                                     (s s + 1) u A
 reflect_pad bwd  up to 9 additions (:182-189)                                                                                 10 u A
Measured on an MI355X (the report of tests/test_gpu_general_sweep.py; max err / bound, max err; the selections are bit-exact, 0):
 bilinear_up_bwd dx     0.221, 4.37e-05   bilinear_up_fwd out    0.85, 3.85e-06   channel_sum out        0.034, 3.94e-05
 dwconv_dgrad dx        0.0992, 7.35e-07   dwconv_fwd y           0.494, 9.48e-07   dwconv_wgrad db        0.0777, 4.80e-06
 dwconv_wgrad dw        0.0875, 8.12e-06   gconv_dgrad dx         0.328, 2.23e-05   gconv_fwd y            0.213, 2.17e-05
 gconv_wgrad db         0.00778, 4.38e-05   gconv_wgrad dw         0.0205, 1.07e-04   gconvt_dgrad dx        0.201, 1.95e-05
 gconvt_fwd y           0.24, 3.38e-06   gconvt_wgrad db        0.00374, 8.96e-06   gconvt_wgrad dw        0.0142, 9.07e-05
 nearest_up_bwd dx      0.307, 8.98e-07   patchconv_dgrad dx     0.994, 1.17e-07   patchconv_fwd y        0.318, 2.29e-06
 patchconv_wgrad db     0.00488, 3.67e-06   patchconv_wgrad dw     0.0417, 1.49e-05   reflect_pad_bwd dx     0.159, 5.85e-07
Every ratio is below 1 and above 1e-3: the smallest belong to the weight- and bias-gradient sums, whose worst-case bound grows with the chain length T while
rounding errors of random sign grow with its root.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
SENT = -1024.0
SENT_U8 = 255
GT, G_OG, G_CC, WG_CC, PC_CHUNKS = 16, 8, 4, 8, 64          # csrc/conv_general.hip :19-21, :180, :374

WORKSPACE_OF = {"gconv_dgrad": "mmif_gconv_dgrad_workspace", "gconv_wgrad": "mmif_gconv_wgrad_workspace", "gconvt_wgrad": "mmif_gconv_wgrad_workspace",
                "patchconv_wgrad": "mmif_patchconv_wgrad_workspace"}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    ep: str                   # the entry point without its mmif_ prefix
    n: int = 1                # samples (planes for the plane-wise resamplers)
    cin: int = 1              # channels of x (the only channel count of the depth-wise kernels and channel_sum)
    cout: int = 1
    h: int = 1                # extent of x (of the ConvTranspose2d's input; relu_bwd: the count; channel_sum: hw)
    w: int = 1
    k: int = 1                # kernel (patch conv: kernel == stride; max-pool: window; nearest: scale)
    s: int = 1
    p: int = 0
    op: int = 0               # output_padding
    reflect: bool = False
    bias: bool = True         # False: NULL
    relu: bool = False
    db: bool = True           # False: NULL
    H: int = 0                # bilinear: output extent
    W: int = 0
    pads: tuple = (0, 0, 0, 0)          # reflect pad: left, right, top, bottom
    plant: str = ""           # windows | ones
    offset: bool = False      # operands start at an odd float offset

    @property
    def id(self):
        s = f"{self.ep}-{self.n}x{self.cin}x{self.h}x{self.w}"
        if self.ep.startswith("gconv"):
            s += f"-o{self.cout}-k{self.k}s{self.s}p{self.p}" + (f"op{self.op}" if "gconvt" in self.ep else ("-reflect" if self.reflect else "-zeros"))
        elif self.ep.startswith("dwconv"):
            s += f"-k{self.k}" + ("-reflect" if self.reflect else "-zeros")
        elif self.ep.startswith(("patchconv", "maxpool", "nearest")):
            s += f"-k{self.k}"
        elif self.ep.startswith("bilinear"):
            s += f"-to{self.H}x{self.W}"
        elif self.ep.startswith("reflect_pad"):
            s += "-pads" + "_".join(str(v) for v in self.pads)
        if self.ep in ("gconv_fwd", "gconvt_fwd", "dwconv_fwd", "patchconv_fwd"):
            s += ("" if self.bias else "-nobias") + ("-relu" if self.relu else "")
        if self.ep.endswith("wgrad") and not self.db:
            s += "-nodb"
        return s + (("-" + self.plant) if self.plant else "") + ("-odd" if self.offset else "")

    # ---- geometry
    @property
    def ho(self):
        return (self.h + 2 * self.p - self.k) // self.s + 1

    @property
    def wo(self):
        return (self.w + 2 * self.p - self.k) // self.s + 1

    @property
    def Ho(self):             # ConvTranspose2d
        return (self.h - 1) * self.s - 2 * self.p + self.k + self.op

    @property
    def Wo(self):
        return (self.w - 1) * self.s - 2 * self.p + self.k + self.op

    @property
    def transposed(self):
        return self.ep.startswith("gconvt")

    def wg(self):
        """(tiles, G, trips) of the weight-gradient launch (mmif_gconv_wgrad :558-559; the transposed alias swaps the channel counts and tiles x)"""
        if self.transposed:
            tiles, pairs = self.n * cdiv(self.h, GT) * cdiv(self.w, GT), cdiv(self.cout, WG_CC) * cdiv(self.cin, G_OG)
        else:
            tiles, pairs = self.n * cdiv(self.ho, GT) * cdiv(self.wo, GT), cdiv(self.cin, WG_CC) * cdiv(self.cout, G_OG)
        G = min(max(1024 // pairs, 1), tiles)
        return tiles, G, cdiv(tiles, G), pairs

    def patch_L(self):
        L = 64
        while L > self.k * self.k:
            L >>= 1
        return L

    def patch_rows(self):
        return self.n * (self.h // self.k)


# ------------------------------------------------------------------------------------------------------------------------------
# float64 building blocks
# ------------------------------------------------------------------------------------------------------------------------------
def refl(t, L):
    """index map of reflect padding without repeating the edge (one fold: |t| < L, t < 2 L - 1)"""
    t = np.abs(np.asarray(t))
    return np.where(t >= L, 2 * (L - 1) - t, t)


def pad2(x, p, mode):
    if p == 0:
        return x
    return np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)), mode={"reflect": "reflect", "symmetric": "symmetric", "zeros": "constant"}[mode])


def corr(xp, w, s, ho, wo, tap_stride=False):
    """xp [n][c][hp][wp], w [o][c][k][k] -> [n][o][ho][wo] = sum w xp[oy s + u][ox s + v]"""
    k = w.shape[2]
    y = np.zeros((xp.shape[0], w.shape[0], ho, wo))
    for u in range(k):
        for v in range(k):
            if tap_stride:          # the wrong definition: oy + u s
                ys, xs = np.clip(np.arange(ho) + u * s, 0, xp.shape[2] - 1), np.clip(np.arange(wo) + v * s, 0, xp.shape[3] - 1)
                win = xp[:, :, ys][:, :, :, xs]
            else:
                win = xp[:, :, u:u + (ho - 1) * s + 1:s, v:v + (wo - 1) * s + 1:s]
            y += np.einsum("oc,nchw->nohw", w[:, :, u, v], win, optimize=True)
    return y


def scatter(g, w, s, hp, wp):
    """the adjoint of corr in xp: g [n][o][ho][wo], w [o][c][k][k] -> [n][c][hp][wp]"""
    k, (ho, wo) = w.shape[2], g.shape[2:]
    z = np.zeros((g.shape[0], w.shape[1], hp, wp))
    for u in range(k):
        for v in range(k):
            z[:, :, u:u + (ho - 1) * s + 1:s, v:v + (wo - 1) * s + 1:s] += np.einsum("oc,nohw->nchw", w[:, :, u, v], g, optimize=True)
    return z


def wcorr(xp, g, k, s):
    """the adjoint of corr in w: [o][c][k][k]"""
    ho, wo = g.shape[2:]
    dw = np.zeros((g.shape[1], xp.shape[1], k, k))
    for u in range(k):
        for v in range(k):
            dw[:, :, u, v] = np.einsum("nohw,nchw->oc", g, xp[:, :, u:u + (ho - 1) * s + 1:s, v:v + (wo - 1) * s + 1:s], optimize=True)
    return dw


def fold_mat(L, p, kind):
    """[L][L + 2p]: which padded positions land on which pixel (reflect: all the images; crop: the direct one)"""
    M = np.zeros((L, L + 2 * p))
    j = np.arange(L + 2 * p)
    if kind == "reflect":
        M[refl(j - p, L), j] = 1.0
    else:
        M[np.arange(L), np.arange(L) + p] = 1.0
    return M


def fold(z, p, h, w, kind):
    """adjoint of the padding: kind reflect | crop | nocorner (the wrong one: the images mirrored in both axes are dropped)"""
    if p == 0:
        return z
    ap = lambda ky, kx: np.einsum("yY,ncYX,xX->ncyx", fold_mat(h, p, ky), z, fold_mat(w, p, kx), optimize=True)
    if kind == "nocorner":
        return ap("reflect", "crop") + ap("crop", "reflect") - ap("crop", "crop")
    return ap(kind, kind)


def bl_weights(h, H, align_false=False):
    """(y0, y1, l, s) per output index; l and s are fp32 values held in float64"""
    Y = np.arange(H)
    if align_false:
        s = np.maximum((Y + 0.5) * h / H - 0.5, 0.0)
        y0 = np.minimum(np.floor(s).astype(np.int64), h - 1)
        return y0, np.minimum(y0 + 1, h - 1), s - y0, s
    r = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0)
    s = (r * Y.astype(np.float32)).astype(np.float32)
    y0 = np.minimum(s.astype(np.int64), h - 1)
    l = (s - y0.astype(np.float32)).astype(np.float32)
    return y0, np.minimum(y0 + 1, h - 1), l.astype(np.float64), s.astype(np.float64)


def bl_mats(h, H, align_false=False):
    """M [H][h] the interpolation map, D [H][h] = d M / d l, cs [H] = u (s + l): what a contracted source coordinate may move l by"""
    y0, y1, l, s = bl_weights(h, H, align_false)
    M, D = np.zeros((H, h)), np.zeros((H, h))
    Y = np.arange(H)
    np.add.at(M, (Y, y0), 1.0 - l)
    np.add.at(M, (Y, y1), l)
    np.add.at(D, (Y, y0), -1.0)
    np.add.at(D, (Y, y1), 1.0)
    return M, D, U * (s + l)


def pool_windows(x, k):
    P, h, w = x.shape
    ho, wo = h // k, w // k
    return x[:, :ho * k, :wo * k].reshape(P, ho, k, wo, k).transpose(0, 1, 3, 2, 4).reshape(P, ho, wo, k * k)


def pad_maps(c, mode="reflect"):
    """row and column index of the source pixel of every output position of the reflect pad / crop"""
    l, r, t, b = c.pads
    H, W = c.h + t + b, c.w + l + r
    if mode == "symmetric":
        f = lambda j, L: np.where(j < 0, -j - 1, np.where(j >= L, 2 * L - 1 - j, j))
    else:
        f = lambda j, L: refl(j, L)
    return f(np.arange(H) - t, c.h), f(np.arange(W) - l, c.w)


def sel_mat(src, L):
    """[len(src)][L] 0/1 map of a gather"""
    M = np.zeros((len(src), L))
    M[np.arange(len(src)), src] = 1.0
    return M


# ------------------------------------------------------------------------------------------------------------------------------
# the result of a definition
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Out:
    name: str
    want: np.ndarray          # float64 (uint8 for dtype u8)
    bound: np.ndarray
    exact: object = False     # a selection, compared bit for bit: True, or a mask of the elements that are
    dtype: str = "f32"
    why_loose: str = ""       # set only where the bound exceeds 1e-3 max |want|: the reason, with the figure behind it
    cond: float = 1.0         # max sum |terms| / max |want| of that output (what why_loose names)


def _o(name, want, T, A, exact=False, why=""):
    """an output whose bound is (T + 1) u A.  Where that exceeds 1e-3 of the largest |want| the reason is recorded: (T + 1) u itself is far below
    1e-3 (asserted by the CPU test), so the excess is the conditioning of the sum, sum |terms| / |sum| = cond, which no bound on a fp32 sum
    can take out"""
    want, A = np.asarray(want, np.float64), np.asarray(A, np.float64)
    if A.ndim and A.shape != want.shape:          # a wrong definition with another extent: only its shape is looked at
        A = np.zeros(want.shape)
    if exact is True:
        return Out(name, want, np.zeros(want.shape), True)
    o = Out(name, want, np.broadcast_to((T + 1) * U * A, want.shape), exact)
    if want.size and np.abs(want).max() > 0 and o.bound.max() > 1e-3 * np.abs(want).max():
        o.cond = float(A.max() / np.abs(want).max())
        o.why_loose = f"{why or 'a cancelling sum'}: sum |terms| is {o.cond:.0f} times the largest |{name}|"
    return o


def compare(o: Out, got):
    """(bad mask, err, err / bound) of a device result against the definition: within the bound, bit-equal where exact, non-finite only where the
    definition is (and then the same)"""
    want = np.asarray(o.want, np.float64).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(o.bound, np.float64), o.want.shape).reshape(-1)
    special = ~np.isfinite(want)
    same_special = np.where(np.isnan(want), np.isnan(got), got == want)
    ok_fin = np.isfinite(got) & ~special
    err = np.where(ok_fin, np.abs(np.where(ok_fin, got, 0.0) - np.where(special, 0.0, want)), np.where(special & same_special, 0.0, np.inf))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    ex = np.broadcast_to(np.asarray(o.exact, bool), o.want.shape).reshape(-1)
    if ex.any() and o.dtype == "f32":
        differ = (got.astype(np.float32).view(np.int32) != want.astype(np.float32).view(np.int32)) & ~np.isnan(want)
        ratio = np.where(ex & differ & (ratio == 0), np.inf, ratio)
    bad = ~(err <= bound) | ~(ratio < np.inf)
    return bad, err, ratio


# ------------------------------------------------------------------------------------------------------------------------------
# definitions, one per entry point: each takes the stored operands and returns [Out]
# ------------------------------------------------------------------------------------------------------------------------------
def _mode(c, mut):
    m = "reflect" if c.reflect else "zeros"
    if mut == "pad_mode_swapped":
        m = "zeros" if c.reflect else "reflect"
    if mut == "reflect_repeats_edge" and c.reflect:
        m = "symmetric"
    return m


def gconv_fwd(c, o, mut=None):
    x, w, b = o["x"], o["w"], o.get("bias")
    ho, wo = c.ho, c.wo
    if mut == "stride2_extent_ceil":
        ho, wo = cdiv(c.h + 2 * c.p - c.k, c.s) + 1, cdiv(c.w + 2 * c.p - c.k, c.s) + 1
        x = np.pad(x, ((0, 0), (0, 0), (0, c.s), (0, c.s)))
    y = corr(pad2(x, c.p, _mode(c, mut)), w, c.s, ho, wo, tap_stride=mut == "stride_on_tap")
    A = corr(pad2(np.abs(o["x"]), c.p, "reflect" if c.reflect else "zeros"), np.abs(w), c.s, c.ho, c.wo)
    if b is not None:
        y, A = y + b.reshape(1, -1, 1, 1), A + np.abs(b).reshape(1, -1, 1, 1)
    if c.relu:
        y = np.maximum(y, 0.0)
    return [_o("y", y, c.cin * c.k * c.k + 1, A)]


def gconv_dgrad(c, o, mut=None):
    gy, w = o["gy"], o["w"]
    hp, wp = c.h + 2 * c.p, c.w + 2 * c.p
    kind = "reflect" if c.reflect else "crop"
    if mut == "dgrad_no_fold":
        kind = "crop"
    if mut == "dgrad_corners_dropped" and c.reflect:
        kind = "nocorner"
    if mut == "pad_mode_swapped":
        kind = "crop" if c.reflect else "reflect"
    dx = fold(scatter(gy, w, c.s, hp, wp), c.p, c.h, c.w, kind)
    A = fold(scatter(np.abs(gy), np.abs(w), c.s, hp, wp), c.p, c.h, c.w, "reflect" if c.reflect else "crop")
    T = c.cout * cdiv(c.k, c.s) ** 2 + 1 + (9 if (c.reflect and c.p > 0) else 0)
    return [_o("dx", dx, T, A, why="a scatter of signed terms cancels")]


def gconv_wgrad(c, o, mut=None):
    x, gy = o["x"], o["gy"]
    tiles, G, trips, _ = c.wg()
    dw = wcorr(pad2(x, c.p, _mode(c, mut)), gy, c.k, c.s)
    A = wcorr(pad2(np.abs(x), c.p, "reflect" if c.reflect else "zeros"), np.abs(gy), c.k, c.s)
    outs = [_o("dw", dw, 256 * trips + G, A, why="a sum over every pixel of every sample cancels")]
    if c.db:
        if mut == "db_over_input_extent":          # the plane walked with the input's extent instead of the output's
            flat = np.concatenate([gy.reshape(-1), np.zeros(c.h * c.w)])
            db = np.array([sum(flat[(i * c.cout + oc) * c.ho * c.wo:][:c.h * c.w].sum() for i in range(c.n)) for oc in range(c.cout)])
        else:
            db = gy.sum((0, 2, 3))
        outs.append(_o("db", db, 256 + trips + G, np.abs(gy).sum((0, 2, 3)), why="a sum over every pixel of every sample cancels"))
    return outs


def _convt_weight(c, w, mut):
    if mut == "convt_weight_co_ci":
        return np.ascontiguousarray(w.reshape(c.cout, c.cin, c.k, c.k).transpose(1, 0, 2, 3))
    if mut == "convt_no_tap_flip":
        return w[:, :, ::-1, ::-1]
    return w


def gconvt_fwd(c, o, mut=None):
    x, w, b = o["x"], o["w"], o.get("bias")
    op = 0 if mut == "convt_no_output_padding" else c.op
    fh, fw = (c.h - 1) * c.s + c.k + op, (c.w - 1) * c.s + c.k + op
    Ho, Wo = c.Ho - c.op + op, c.Wo - c.op + op
    y = scatter(x, _convt_weight(c, w, mut), c.s, fh, fw)[:, :, c.p:c.p + Ho, c.p:c.p + Wo]
    A = scatter(np.abs(x), np.abs(w), c.s, fh + c.op - op, fw + c.op - op)[:, :, c.p:c.p + c.Ho, c.p:c.p + c.Wo]
    if b is not None:
        y, A = y + b.reshape(1, -1, 1, 1), A + np.abs(b).reshape(1, -1, 1, 1)
    if c.relu:
        y = np.maximum(y, 0.0)
    return [_o("y", y, c.cin * cdiv(c.k, c.s) ** 2 + 1, A, why="a scatter of signed terms cancels")]


def _embed(c, gy):
    """gy on the un-cropped domain of the transposed conv's scatter"""
    full = np.zeros(gy.shape[:2] + ((c.h - 1) * c.s + c.k + c.op, (c.w - 1) * c.s + c.k + c.op))
    full[:, :, c.p:c.p + c.Ho, c.p:c.p + c.Wo] = gy
    return full


def gconvt_dgrad(c, o, mut=None):
    gy, w = o["gy"], _convt_weight(c, o["w"], mut)
    dx = corr(_embed(c, gy), w, c.s, c.h, c.w)
    A = corr(_embed(c, np.abs(gy)), np.abs(o["w"]), c.s, c.h, c.w)
    return [_o("dx", dx, c.cout * c.k * c.k, A)]


def gconvt_wgrad(c, o, mut=None):
    x, gy = o["x"], o["gy"]
    tiles, G, trips, _ = c.wg()
    dw = wcorr(_embed(c, gy), x, c.k, c.s)
    if mut == "convt_no_tap_flip":
        dw = dw[:, :, ::-1, ::-1]
    A = wcorr(_embed(c, np.abs(gy)), np.abs(x), c.k, c.s)
    outs = [_o("dw", dw, 256 * trips + G, A, why="a sum over every pixel of every sample cancels")]
    if c.db:
        outs.append(_o("db", x.sum((0, 2, 3)), 256 + trips + G, np.abs(x).sum((0, 2, 3)), why="a sum over every pixel of every sample cancels"))
    return outs


def relu_bwd(c, o, mut=None):
    keep = (o["y"] >= 0) if mut == "relu_ge_zero" else (o["y"] > 0)
    return [_o("out", np.where(keep, o["g"], 0.0), 0, 0.0, exact=True)]


def channel_sum(c, o, mut=None):
    x = o["x"]
    return [_o("out", x.sum((0, 2)), c.n * cdiv(c.h, 256) + 10, np.abs(x).sum((0, 2)), why="a sum over every pixel of every sample cancels")]


def _dw_weight(c, w, mut):
    return np.broadcast_to(w[:1], w.shape) if mut == "dw_shared_weights" else w


def dwconv_fwd(c, o, mut=None):
    x, w, b = o["x"], _dw_weight(c, o["w"], mut), o.get("bias")
    p = c.k // 2
    xp, ap = pad2(x, p, _mode(c, mut)), pad2(np.abs(x), p, "reflect" if c.reflect else "zeros")
    y, A = np.zeros(x.shape), np.zeros(x.shape)
    for u in range(c.k):
        for v in range(c.k):
            y += xp[:, :, u:u + c.h, v:v + c.w] * w[None, :, 0, u, v, None, None]
            A += ap[:, :, u:u + c.h, v:v + c.w] * np.abs(o["w"])[None, :, 0, u, v, None, None]
    if b is not None:
        y, A = y + b.reshape(1, -1, 1, 1), A + np.abs(b).reshape(1, -1, 1, 1)
    return [_o("y", y, c.k * c.k, A)]


def dwconv_dgrad(c, o, mut=None):
    gy, w = o["gy"], _dw_weight(c, o["w"], mut)
    p = c.k // 2
    z, za = np.zeros(gy.shape[:2] + (c.h + 2 * p, c.w + 2 * p)), np.zeros(gy.shape[:2] + (c.h + 2 * p, c.w + 2 * p))
    for u in range(c.k):
        for v in range(c.k):
            z[:, :, u:u + c.h, v:v + c.w] += gy * w[None, :, 0, u, v, None, None]
            za[:, :, u:u + c.h, v:v + c.w] += np.abs(gy) * np.abs(o["w"])[None, :, 0, u, v, None, None]
    kind = "reflect" if c.reflect else "crop"
    if mut == "dw_dgrad_no_mirror":
        kind = "crop"
    if mut == "pad_mode_swapped":
        kind = "crop" if c.reflect else "reflect"
    return [_o("dx", fold(z, p, c.h, c.w, kind), 9 * c.k * c.k, fold(za, p, c.h, c.w, "reflect" if c.reflect else "crop"))]


def dwconv_wgrad(c, o, mut=None):
    x, gy = o["x"], o["gy"]
    p = c.k // 2
    xp, ap = pad2(x, p, _mode(c, mut)), pad2(np.abs(x), p, "reflect" if c.reflect else "zeros")
    dw, A = np.zeros((c.cin, 1, c.k, c.k)), np.zeros((c.cin, 1, c.k, c.k))
    for u in range(c.k):
        for v in range(c.k):
            dw[:, 0, u, v] = (gy * xp[:, :, u:u + c.h, v:v + c.w]).sum((0, 2, 3))
            A[:, 0, u, v] = (np.abs(gy) * ap[:, :, u:u + c.h, v:v + c.w]).sum((0, 2, 3))
    if mut == "dw_shared_weights":
        dw = np.broadcast_to(dw.sum(0, keepdims=True), dw.shape)
    T = c.n * cdiv(c.h * c.w, 256) + 10
    outs = [_o("dw", dw, T, A, why="a sum over every pixel of every sample cancels")]
    if c.db:
        outs.append(_o("db", gy.sum((0, 2, 3)), T, np.abs(gy).sum((0, 2, 3)), why="a sum over every pixel of every sample cancels"))
    return outs


def _patches(c, x):
    """[n][c][oh][ow][s][s] of the covered area"""
    s, oh, ow = c.k, c.h // c.k, c.w // c.k
    return x[:, :, :oh * s, :ow * s].reshape(c.n, c.cin, oh, s, ow, s).transpose(0, 1, 2, 4, 3, 5)


def _patch_weight(c, w, mut):
    return np.ascontiguousarray(w.transpose(0, 1, 3, 2)) if mut == "patch_taps_transposed" else w


def patchconv_fwd(c, o, mut=None):
    x, w, b = o["x"], _patch_weight(c, o["w"], mut), o.get("bias")
    y = np.einsum("nchwuv,cuv->nchw", _patches(c, x), w[:, 0])
    A = np.einsum("nchwuv,cuv->nchw", _patches(c, np.abs(x)), np.abs(o["w"])[:, 0])
    if b is not None:
        y, A = y + b.reshape(1, -1, 1, 1), A + np.abs(b).reshape(1, -1, 1, 1)
    L = c.patch_L()
    return [_o("y", y, cdiv(c.k * c.k, L) + int(np.log2(L)) + 1, A)]


def patchconv_dgrad(c, o, mut=None):
    gy, w = o["gy"], _patch_weight(c, o["w"], mut)
    s, oh, ow = c.k, c.h // c.k, c.w // c.k
    ys, xs = np.arange(c.h), np.arange(c.w)
    oy, ox = np.minimum(ys // s, oh - 1), np.minimum(xs // s, ow - 1)
    dx = gy[:, :, oy][:, :, :, ox] * w[:, 0][:, ys % s][:, :, xs % s][None]
    covered = (ys < oh * s)[:, None] & (xs < ow * s)[None, :]
    if mut != "patch_remainder_neighbour":
        dx = np.where(covered, dx, 0.0)
    exact = np.broadcast_to(~covered, dx.shape)
    return [Out("dx", dx, np.where(exact, 0.0, U * np.abs(dx)), exact)]


def patchconv_wgrad(c, o, mut=None):
    x, gy = o["x"], o["gy"]
    dw = np.einsum("nchwuv,nchw->cuv", _patches(c, x), gy)[:, None]
    if mut == "patch_taps_transposed":
        dw = np.ascontiguousarray(dw.transpose(0, 1, 3, 2))
    A = np.einsum("nchwuv,nchw->cuv", _patches(c, np.abs(x)), np.abs(gy))[:, None]
    per, lanes = cdiv(c.patch_rows(), PC_CHUNKS), 256 // (c.k * c.k)
    T = cdiv(per * (c.w // c.k), lanes) + lanes + PC_CHUNKS
    outs = [_o("dw", dw, T, A, why="a sum over every patch of every sample cancels")]
    if c.db:
        outs.append(_o("db", gy.sum((0, 2, 3)), T, np.abs(gy).sum((0, 2, 3)), why="a sum over every patch of every sample cancels"))
    return outs


def bilinear_up_fwd(c, o, mut=None):
    x = o["x"]
    af = mut == "bilinear_align_corners_false"
    (My, Dy, cy), (Mx, Dx, cx) = bl_mats(c.h, c.H, af), bl_mats(c.w, c.W, af)
    y = np.einsum("Yy,pyx,Xx->pYX", My, x, Mx)
    (My, Dy, cy), (Mx, Dx, cx) = bl_mats(c.h, c.H), bl_mats(c.w, c.W)
    A = np.einsum("Yy,pyx,Xx->pYX", My, np.abs(x), Mx)
    bound = 7 * U * A + cy[None, :, None] * np.abs(np.einsum("Yy,pyx,Xx->pYX", Dy, x, Mx)) + cx[None, None, :] * np.abs(np.einsum("Yy,pyx,Xx->pYX", My, x, Dx))
    return [Out("out", y, bound)]


def bilinear_up_bwd(c, o, mut=None):
    g = o["g"]
    (My, Dy, cy), (Mx, Dx, cx) = bl_mats(c.h, c.H), bl_mats(c.w, c.W)
    Mx_used = Mx
    if mut == "bilinear_bwd_transpose_one_axis":          # the x axis averaged back instead of transposed
        Mx_used = Mx / Mx.sum(0, keepdims=True)
    dx = np.einsum("Yy,pYX,Xx->pyx", My, g, Mx_used)
    A = np.einsum("Yy,pYX,Xx->pyx", My, np.abs(g), Mx)
    T = int((Mx != 0).sum(0).max() + (My != 0).sum(0).max()) + 3
    bound = (T + 1) * U * A + np.einsum("Yy,pYx->pyx", np.abs(Dy) * cy[:, None], np.abs(np.einsum("pYX,Xx->pYx", g, Mx))) + \
        np.einsum("Xx,pyX->pyx", np.abs(Dx) * cx[:, None], np.abs(np.einsum("Yy,pYX->pyX", My, g)))
    return [Out("dx", dx, bound)]


def maxpool_nchw_fwd(c, o, mut=None):
    x, k = o["x"], c.k
    if mut == "maxpool_ceil_mode":
        x = np.pad(x, ((0, 0), (0, (-c.h) % k), (0, (-c.w) % k)), constant_values=-np.inf)
    win = pool_windows(x, k)
    idx = (k * k - 1 - np.argmax(win[..., ::-1], -1)) if mut == "maxpool_last_max" else np.argmax(win, -1)          # (argmax: the first NaN, else the first maximum)
    y = np.take_along_axis(win, idx[..., None], -1)[..., 0]
    return [_o("y", y, 0, 0.0, exact=True), Out("idx", idx.astype(np.uint8), np.zeros(idx.shape), True, "u8")]


def maxpool_nchw_bwd(c, o, mut=None):
    g, idx, k = o["g"], o["idx"].astype(np.int64), c.k
    ho, wo = c.h // k, c.w // k
    dx = np.zeros((c.n, c.h, c.w))
    P, Y, X = np.meshgrid(np.arange(c.n), np.arange(ho), np.arange(wo), indexing="ij")
    dx[P, Y * k + idx // k, X * k + idx % k] = g
    return [_o("dx", dx, 0, 0.0, exact=True)]


def nearest_up_fwd(c, o, mut=None):
    s = c.k
    return [_o("y", o["x"][:, np.arange(c.h * s) // s][:, :, np.arange(c.w * s) // s], 0, 0.0, exact=True)]


def nearest_up_bwd(c, o, mut=None):
    s, g = c.k, o["g"]
    r = lambda a: a.reshape(c.n, c.h, s, c.w, s).sum((2, 4))
    dx = r(g) / (s * s if mut == "nearest_bwd_mean" else 1)
    return [_o("dx", dx, s * s, r(np.abs(g)), exact=(s == 1))] if s > 1 else [_o("dx", dx, 0, 0.0, exact=True)]


def reflect_pad_fwd(c, o, mut=None):
    ry, rx = pad_maps(c, "symmetric" if mut == "reflect_repeats_edge" else "reflect")
    return [_o("y", o["x"][:, ry][:, :, rx], 0, 0.0, exact=True)]


def reflect_pad_bwd(c, o, mut=None):
    g = o["g"]
    ry, rx = pad_maps(c)
    My, Mx = sel_mat(ry, c.h), sel_mat(rx, c.w)
    A = np.einsum("Yy,pYX,Xx->pyx", My, np.abs(g), Mx)
    if mut == "reflect_bwd_edge_twice":          # the edge row counted as its own mirror
        l, r, t, b = c.pads
        My = My.copy()
        if t > 0:
            My[t, 0] += 1.0
        if b > 0:
            My[t + c.h - 1, c.h - 1] += 1.0
    return [_o("dx", np.einsum("Yy,pYX,Xx->pyx", My, g, Mx), 9, A)]


DEFS = dict(gconv_fwd=gconv_fwd, gconv_dgrad=gconv_dgrad, gconv_wgrad=gconv_wgrad, gconvt_fwd=gconvt_fwd, gconvt_dgrad=gconvt_dgrad,
            gconvt_wgrad=gconvt_wgrad, relu_bwd=relu_bwd, channel_sum=channel_sum, dwconv_fwd=dwconv_fwd, dwconv_dgrad=dwconv_dgrad,
            dwconv_wgrad=dwconv_wgrad, patchconv_fwd=patchconv_fwd, patchconv_dgrad=patchconv_dgrad, patchconv_wgrad=patchconv_wgrad,
            bilinear_up_fwd=bilinear_up_fwd, bilinear_up_bwd=bilinear_up_bwd, maxpool_nchw_fwd=maxpool_nchw_fwd, maxpool_nchw_bwd=maxpool_nchw_bwd,
            nearest_up_fwd=nearest_up_fwd, nearest_up_bwd=nearest_up_bwd, reflect_pad_fwd=reflect_pad_fwd, reflect_pad_bwd=reflect_pad_bwd)
EPS = tuple(DEFS)


def define(c: Case, mut=None, o=None):
    """[Out] of everything the case's call writes (o: other stored operands than the case's own, for the chained checks)"""
    return DEFS[c.ep](c, operands(c) if o is None else o, mut)


# wrong definitions: name -> (entry points it can show on, which of their cases)
MUTATIONS = {
    "reflect_repeats_edge": (("gconv_fwd", "gconv_wgrad", "dwconv_fwd", "reflect_pad_fwd"), lambda c: (c.reflect and c.p > 0) or (c.ep.startswith("dw") and c.reflect and c.k == 3) or max(c.pads) > 0),
    "pad_mode_swapped": (("gconv_fwd", "gconv_dgrad", "gconv_wgrad", "dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"), lambda c: min(c.h, c.w) > c.p > 0 or (c.ep.startswith("dw") and c.k == 3 and min(c.h, c.w) > 1)),
    "stride_on_tap": (("gconv_fwd",), lambda c: c.s == 2 and c.k > 1 and c.ho > 1),
    "stride2_extent_ceil": (("gconv_fwd",), lambda c: c.s == 2 and (c.h + 2 * c.p - c.k) % 2 == 1),
    "dgrad_no_fold": (("gconv_dgrad",), lambda c: c.reflect and c.p > 0),
    "dgrad_corners_dropped": (("gconv_dgrad",), lambda c: c.reflect and c.p > 0),
    "db_over_input_extent": (("gconv_wgrad",), lambda c: c.db and c.ho * c.wo < c.h * c.w),
    "convt_no_output_padding": (("gconvt_fwd",), lambda c: c.op > 0),
    "convt_weight_co_ci": (("gconvt_fwd", "gconvt_dgrad"), lambda c: c.cin * c.cout > 1),
    "convt_no_tap_flip": (("gconvt_fwd", "gconvt_dgrad", "gconvt_wgrad"), lambda c: c.k > 1),
    "dw_shared_weights": (("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"), lambda c: c.cin > 1),
    "dw_dgrad_no_mirror": (("dwconv_dgrad",), lambda c: c.reflect and c.k == 3),
    "patch_taps_transposed": (("patchconv_fwd", "patchconv_dgrad", "patchconv_wgrad"), lambda c: True),
    "patch_remainder_neighbour": (("patchconv_dgrad",), lambda c: c.h % c.k or c.w % c.k),
    "bilinear_align_corners_false": (("bilinear_up_fwd",), lambda c: c.H > c.h > 1 or c.W > c.w > 1),
    "bilinear_bwd_transpose_one_axis": (("bilinear_up_bwd",), lambda c: c.W > c.w),
    "maxpool_last_max": (("maxpool_nchw_fwd",), lambda c: c.k > 1),
    "maxpool_ceil_mode": (("maxpool_nchw_fwd",), lambda c: c.h % c.k or c.w % c.k),
    "nearest_bwd_mean": (("nearest_up_bwd",), lambda c: c.k > 1),
    "reflect_bwd_edge_twice": (("reflect_pad_bwd",), lambda c: c.pads[2] > 0 or c.pads[3] > 0),
    "relu_ge_zero": (("relu_bwd",), lambda c: c.h >= 255),
}


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
_OPS = {}
RELU_PLANTS = (0.0, -0.0, 2.0 ** -149, 2.0 ** -126)          # +0.0, -0.0, the smallest positive fp32 (a denormal), the smallest normal


def maxpool_plants(c):
    """window -> what is planted there (plant == 'windows': plane 0)"""
    return {(0, 0): "all_neg_inf", (0, 1): "signed_zeros", (1, 0): "one_nan_not_first", (1, 1): "all_nan"} if c.plant == "windows" else {}


def operands(c: Case) -> dict:
    if c.id in _OPS:
        return _OPS[c.id]
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    N = lambda *shape, scale=1.0: f32(scale * rng.standard_normal(shape))
    o = {}
    ep = c.ep
    if ep.startswith("gconvt"):
        wshape = (c.cin, c.cout, c.k, c.k)
        if ep != "gconvt_dgrad":
            o["x"] = N(c.n, c.cin, c.h, c.w)
        if ep != "gconvt_wgrad":
            o["w"] = N(*wshape, scale=0.5)
        if ep == "gconvt_fwd" and c.bias:
            o["bias"] = N(c.cout)
        if ep != "gconvt_fwd":
            o["gy"] = N(c.n, c.cout, c.Ho, c.Wo)
    elif ep.startswith("gconv"):
        if ep != "gconv_dgrad":
            o["x"] = N(c.n, c.cin, c.h, c.w)
        if ep != "gconv_wgrad":
            o["w"] = N(c.cout, c.cin, c.k, c.k, scale=0.5)
        if ep == "gconv_fwd" and c.bias:
            o["bias"] = N(c.cout)
        if ep != "gconv_fwd":
            o["gy"] = N(c.n, c.cout, c.ho, c.wo)
    elif ep == "relu_bwd":
        o["g"], o["y"] = N(c.h), N(c.h)
        for j in range(min(c.h, 16)):
            i = (j * 37) % c.h
            o["y"][i] = RELU_PLANTS[j % 4]
            o["g"][i] = f32(0.5 + abs(o["g"][i])) * (-1.0 if j % 3 == 0 else 1.0)
        if c.h > 20:
            o["g"][5] = -0.0          # a signed zero that passes (y[5] is left as drawn unless planted; either way the bits are compared)
    elif ep == "channel_sum":
        o["x"] = N(c.n, c.cin, c.h) + f32(0.25)
        o["x"] = f32(o["x"])
    elif ep.startswith("dwconv"):
        if ep != "dwconv_dgrad":
            o["x"] = N(c.n, c.cin, c.h, c.w)
        if ep != "dwconv_wgrad":
            o["w"] = N(c.cin, 1, c.k, c.k, scale=0.5)
        if ep == "dwconv_fwd" and c.bias:
            o["bias"] = N(c.cin)
        if ep != "dwconv_fwd":
            o["gy"] = N(c.n, c.cin, c.h, c.w)
    elif ep.startswith("patchconv"):
        if ep != "patchconv_dgrad":
            o["x"] = N(c.n, c.cin, c.h, c.w)
        if ep != "patchconv_wgrad":
            o["w"] = N(c.cin, 1, c.k, c.k, scale=0.5)
        if ep == "patchconv_fwd" and c.bias:
            o["bias"] = N(c.cin)
        if ep != "patchconv_fwd":
            o["gy"] = N(c.n, c.cin, c.h // c.k, c.w // c.k)
    elif ep == "bilinear_up_fwd":
        o["x"] = N(c.n, c.h, c.w)
    elif ep == "bilinear_up_bwd":
        o["g"] = np.ones((c.n, c.H, c.W)) if c.plant == "ones" else N(c.n, c.H, c.W)
    elif ep.startswith("maxpool"):
        x = rng.integers(-3, 4, (c.n, c.h, c.w)).astype(np.float64)          # small integers: many ties
        k = c.k
        for (wy, wx), what in maxpool_plants(c).items():
            blk = x[0, wy * k:(wy + 1) * k, wx * k:(wx + 1) * k]
            if what == "all_neg_inf":
                blk[:] = -np.inf
            elif what == "signed_zeros":          # -0.0 before +0.0, everything else below
                b = np.full(k * k, -1.0)
                b[1], b[k * k - 1] = -0.0, 0.0
                blk[:] = b.reshape(k, k)
            elif what == "one_nan_not_first":
                blk[0, 1] = np.nan
            else:
                blk[:] = np.nan
        if ep == "maxpool_nchw_fwd":
            o["x"] = x
        else:
            o["idx"] = maxpool_nchw_fwd(c, {"x": x})[1].want
            o["g"] = N(c.n, c.h // k, c.w // k)
    elif ep == "nearest_up_fwd":
        o["x"] = N(c.n, c.h, c.w)
    elif ep == "nearest_up_bwd":
        o["g"] = N(c.n, c.h * c.k, c.w * c.k)
    elif ep == "reflect_pad_fwd":
        o["x"] = N(c.n, c.h, c.w)
    elif ep == "reflect_pad_bwd":
        l, r, t, b = c.pads
        o["g"] = N(c.n, c.h + t + b, c.w + l + r)
    else:
        raise KeyError(ep)
    _OPS[c.id] = o
    while len(_OPS) > 8:
        _OPS.pop(next(iter(_OPS)))
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
EXTENTS = (1, 15, 16, 17, 33)
CINS = (1, 3, 4, 5, 9)
COUTS = (1, 7, 8, 9, 17)
WG_CINS = (7, 8, 9)
GEOMS = [(k, s, p) for k, ps in ((1, (0,)), (3, (0, 1)), (5, (0, 1, 2)), (7, (0, 2, 3))) for s in (1, 2) for p in ps]
CONVT_GEOMS = ((3, 2, 1, 1), (3, 2, 1, 0), (3, 1, 1, 0), (5, 2, 2, 1), (1, 2, 0, 1), (7, 2, 3, 0))
RELU_COUNTS = (0, 1, 255, 256, 257)
SUM_HW = (1, 255, 256, 257, 1000)
DW_HW = ((2, 2), (2, 9), (17, 16), (1, 257))
PATCH_S = (2, 3, 4, 7, 8, 11, 16)
PATCH_ROWS = {1: (1, 1), 63: (3, 21), 64: (2, 32), 65: (5, 13), 130: (2, 65)}          # n (h / s) -> (n, h / s)
BILINEAR = ((1, 1), (1, 4), (2, 2), (3, 4), (5, 13), (7, 56), (33, 264))
POOL_K = (1, 2, 3, 4, 15)
NEAREST_HW = ((1, 1), (3, 2), (5, 7))
PADS = [((1, 1), (0, 0, 0, 0)), ((2, 2), (1, 0, 0, 0)), ((2, 2), (0, 1, 0, 0)), ((2, 2), (0, 0, 1, 0)), ((2, 2), (0, 0, 0, 1)), ((2, 2), (1, 1, 1, 1)),
        ((3, 5), (4, 0, 0, 0)), ((3, 5), (0, 4, 0, 0)), ((3, 5), (0, 0, 2, 0)), ((3, 5), (0, 0, 0, 2)), ((3, 5), (4, 4, 2, 2)), ((3, 5), (0, 0, 0, 0)),
        ((6, 7), (-2, 0, 0, 0)), ((6, 7), (0, -3, 0, 0)), ((6, 7), (0, 0, -1, 0)), ((6, 7), (0, 0, 0, -4)), ((6, 7), (6, -2, -1, 5)), ((6, 7), (-1, 3, 4, -2)),
        ((6, 7), (6, 6, 5, 5)), ((3, 5), (-1, -1, -1, -1))]


def _in_extent(out, k, s, p, parity):
    """the input extent that gives `out` outputs, with (h + 2p - k) % s == parity"""
    return (out - 1) * s + k - 2 * p + (parity if s == 2 else 0)


def _cases():
    cs = []
    i = 0
    # ---- general conv: every geometry x padding mode, the three entry points, extents / channels / flags / batch in rotation
    for (k, s, p) in GEOMS:
        for reflect in (False, True):
            if reflect and p == 0:
                continue
            for ep in ("gconv_fwd", "gconv_dgrad", "gconv_wgrad"):
                ho, wo = EXTENTS[i % 5], EXTENTS[(i // 5 + i + 2) % 5]
                if ho == wo:
                    wo = EXTENTS[(EXTENTS.index(wo) + 1) % 5]
                h, w = _in_extent(ho, k, s, p, i % 2), _in_extent(wo, k, s, p, (i // 2) % 2)
                while h < 1 or (reflect and h <= p):
                    ho += 1
                    h = _in_extent(ho, k, s, p, i % 2)
                while w < 1 or (reflect and w <= p):
                    wo += 1
                    w = _in_extent(wo, k, s, p, (i // 2) % 2)
                cin = WG_CINS[i % 3] if ep == "gconv_wgrad" else CINS[(i // 3) % 5]
                cs.append(Case(ep, n=(1, 3)[i % 2], cin=cin, cout=COUTS[(i // 2 + i // 7) % 5], h=h, w=w, k=k, s=s, p=p, reflect=reflect,
                               bias=bool((i // 3) % 2), relu=bool((i // 6) % 2), db=bool((i // 3) % 2), offset=i % 4 == 1))
                i += 1
    # ---- the smallest legal reflect inputs (h = p + 1): every fold clause alone and together
    for j, (k, p, h, w) in enumerate(((3, 1, 2, 2), (5, 2, 3, 3), (7, 3, 4, 4), (5, 2, 3, 6), (7, 3, 9, 4), (5, 1, 3, 4), (7, 2, 3, 3))):
        for s in (1, 2):
            for ep in ("gconv_fwd", "gconv_dgrad", "gconv_wgrad"):
                cs.append(Case(ep, n=2, cin=8 if ep == "gconv_wgrad" else 3, cout=7, h=h, w=w, k=k, s=s, p=p, reflect=True, offset=(j + s) % 4 == 0))
    # ---- the extents, cin and cout the rotation left out for an entry point
    for ep in ("gconv_fwd", "gconv_dgrad", "gconv_wgrad"):
        mine = [c for c in cs if c.ep == ep]
        out_ext = {c.ho for c in mine} | {c.wo for c in mine}
        for j, e in enumerate(x for x in EXTENTS if x not in out_ext):
            cs.append(Case(ep, n=1, cin=8 if ep == "gconv_wgrad" else 3, cout=9, h=e, w=e + 2, k=3, s=1, p=1, reflect=bool(j % 2)))
        for j, ci in enumerate(x for x in (WG_CINS if ep == "gconv_wgrad" else CINS) if x not in {c.cin for c in mine}):
            cs.append(Case(ep, n=1, cin=ci, cout=8, h=17, w=9, k=3, s=1 + j % 2, p=1, reflect=True))
        for j, co in enumerate(x for x in COUTS if x not in {c.cout for c in mine}):
            cs.append(Case(ep, n=1, cin=8 if ep == "gconv_wgrad" else 4, cout=co, h=9, w=17, k=3, s=1 + j % 2, p=1, reflect=False))
    # ---- weight gradient: more than one trip of the tile loop with a ragged last one (9 tiles on 8 groups; 18 tiles on 8 groups), and
    #      pairs > 1024 on one tile and on several; the same two edges through the transposed alias, whose tiles are those of x
    cs.append(Case("gconv_wgrad", n=1, cin=64, cout=128, h=48, w=48, k=3, s=1, p=1, reflect=True))
    cs.append(Case("gconv_wgrad", n=3, cin=56, cout=136, h=65, w=33, k=3, s=2, p=1, reflect=False, db=False, offset=True))
    cs.append(Case("gconv_wgrad", n=1, cin=265, cout=249, h=5, w=6, k=1, s=1, p=0))
    cs.append(Case("gconv_wgrad", n=2, cin=265, cout=249, h=18, w=17, k=1, s=1, p=0, db=False))
    cs.append(Case("gconvt_wgrad", n=1, cin=128, cout=64, h=48, w=48, k=3, s=2, p=1, op=1, db=False))
    cs.append(Case("gconvt_wgrad", n=2, cin=249, cout=265, h=5, w=18, k=1, s=2, p=0, op=1, offset=True))
    # ---- ConvTranspose2d: the six geometries, two rounds of extents; channels and flags rotate on a counter of the entry point's own
    for rnd in range(2):
        for j, (k, s, p, op) in enumerate(CONVT_GEOMS):
            for e, ep in enumerate(("gconvt_fwd", "gconvt_dgrad", "gconvt_wgrad")):
                t = rnd * 6 + j          # 0..11 per entry point
                h, w = ((1, 9), (8, 17), (9, 2), (17, 8), (5, 16), (16, 1))[(t + e + rnd) % 6]
                cin = WG_CINS[t % 3] if ep == "gconvt_wgrad" else CINS[(t + e) % 5]
                cs.append(Case(ep, n=(3, 1)[t % 2], cin=cin, cout=COUTS[(t // 2 + t + e) % 5], h=h, w=w, k=k, s=s, p=p, op=op, bias=bool((t // 2) % 2),
                               relu=bool(t % 2), db=bool((t // 3) % 2), offset=(t + e) % 4 == 2))
    # ---- ReLU backward, channel sum
    for j, cnt in enumerate(RELU_COUNTS):
        cs.append(Case("relu_bwd", h=cnt, offset=j % 2 == 1))
    for j, hw in enumerate(SUM_HW):
        for c in (1, 5):
            cs.append(Case("channel_sum", n=3, cin=c, h=hw, offset=(j + c) % 4 == 0))
    # ---- depth-wise
    for ep in ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"):
        for k in (1, 3):
            for reflect in (False, True):
                for flag in (False, True):
                    for (h, w) in DW_HW[:4 if k == 1 else 3]:
                        if not flag and (h, w) in ((2, 9),):
                            continue
                        cs.append(Case(ep, n=3, cin=(1, 3, 5)[i % 3], h=h, w=w, k=k, reflect=reflect, bias=flag, db=flag, offset=i % 4 == 3))
                        i += 1
    # ---- patch conv
    for j, s in enumerate(PATCH_S):
        for rem in (0, 1):
            h, w = s * (2 + j % 2) + rem * (s - 1), s * (3 - j % 2) + rem * (1 + j % (s - 1))
            cs.append(Case("patchconv_fwd", n=2, cin=(3, 1, 5)[j % 3], h=h, w=w, k=s, bias=bool((j + rem) % 2), offset=(j + rem) % 4 == 0))
            cs.append(Case("patchconv_dgrad", n=2, cin=(1, 5, 3)[j % 3], h=h, w=w, k=s, offset=(j + rem) % 4 == 1))
        for r2, rows in enumerate((tuple(PATCH_ROWS)[j % 5], tuple(PATCH_ROWS)[(j + 2) % 5], tuple(PATCH_ROWS)[(j + 3) % 5])):
            n, oh = PATCH_ROWS[rows]
            cs.append(Case("patchconv_wgrad", n=n, cin=(2, 3)[(j + r2) % 2], h=oh * s + (r2 * (s - 1)) % s, w=s * (1 + (j + r2) % 3) + (j % 2), k=s,
                           db=bool((j + r2) % 2), offset=(j + r2) % 4 == 2))
    # ---- bilinear through the C ABI: H, W free, the axes mixed
    for j, (h, H) in enumerate(BILINEAR):
        w, W = BILINEAR[(j + 3) % 7]
        if h == 33 or h == 1 and H == 4:
            w, W = (7, 56) if h == 33 else (5, 13)          # keep H W small where the backward's candidate window is the whole axis
        for planes in (1, 6):
            if (planes == 6) != (j % 2 == 0) and h not in (1, 2):
                continue
            cs.append(Case("bilinear_up_fwd", n=planes, h=h, w=w, H=H, W=W, offset=j % 4 == 1))
            cs.append(Case("bilinear_up_bwd", n=planes, h=h, w=w, H=H, W=W, offset=j % 4 == 3))
        cs.append(Case("bilinear_up_bwd", n=1, h=h, w=w, H=H, W=W, plant="ones"))
    # ---- max-pool
    for j, k in enumerate(POOL_K):
        for rem in (0, 1):
            h, w = k * (2 + j % 2) + rem * (k - 1), k * (3 - j % 2) + rem * max(k // 2, 1 if k > 1 else 0)
            if k == 1 and rem:
                h, w = 5, 7
            for ep in ("maxpool_nchw_fwd", "maxpool_nchw_bwd"):
                cs.append(Case(ep, n=(1, 6)[(j + rem) % 2], h=h, w=w, k=k, plant="windows" if k > 1 else "", offset=(j + rem) % 4 == 0))
    # ---- nearest
    for s in (1, 2, 3, 4):
        for j, (h, w) in enumerate(NEAREST_HW):
            for ep in ("nearest_up_fwd", "nearest_up_bwd"):
                cs.append(Case(ep, n=(1, 6)[(s + j) % 2], h=h, w=w, k=s, offset=(s + j) % 4 == 0))
    # ---- reflect pad / crop
    for j, ((h, w), pads) in enumerate(PADS):
        for ep in ("reflect_pad_fwd", "reflect_pad_bwd"):
            cs.append(Case(ep, n=(1, 6)[j % 2], h=h, w=w, pads=pads, offset=j % 4 == 1))
    return cs


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


def elements(c: Case):
    """the largest tensor of the case"""
    o = operands(c)
    return max([np.asarray(v).size for v in o.values()] + [d.want.size for d in define(c)])
