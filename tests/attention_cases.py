"""Cases and numpy float64 restatements (explicit backward formulas) for golden F24: the multi-head spatial-reduction attention of
reference core/block.py:355-434 and the blocks built on it (LayerNorm :472-500, MetaFormerBlock :503-540, TransformerBlock :603-617,
TransitionBlock :620-664).

The fixture tests/golden/f24_attention.npz (written by tests/golden/make_golden_attention.py from the reference's own modules in
float64) holds results only; inputs and parameters are rebuilt here from seeds and are float32-exact, so that the fp32 kernels and the
float64 oracles start from the same numbers.  Gradients are those of sum(y * upstream).  Arrays of more than SAMPLE_ABOVE elements are
stored as a flat strided sample (sample_index); the restatements below are pinned to those samples on the CPU and then serve as the
full-tensor float64 reference of the GPU tests.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F24 = os.path.join(HERE, "golden", "f24_attention.npz")
F24_MANIFEST = os.path.join(HERE, "golden", "f24_manifest.json")
SAMPLE_ABOVE = 600


def sample_index(size):
    """flat indices a stored array holds: all of them up to SAMPLE_ABOVE elements, else every k-th with k odd"""
    if size <= SAMPLE_ABOVE:
        return np.arange(size)
    k = -(-size // SAMPLE_ABOVE) | 1
    return np.arange(0, size, k)


def _f32(a):
    return np.asarray(a, np.float32)


# ------------------------------------------------------------------ the attention core
# name -> (B, heads, d, N, M, seed, gain): q and k are standard normal times gain
CORE_CASES = {
    "n740_m2": (1, 1, 16, 740, 2, 2401, 1.0),        # ragged N, one partial key tile
    "m1": (1, 1, 16, 256, 1, 2402, 1.0),             # softmax of one key: o = v, dq = dk = 0
    "h2_m6": (2, 2, 16, 384, 6, 2403, 1.0),          # two heads, six keys
    "h3_m17": (1, 3, 16, 132, 17, 2404, 1.0),        # a full key tile plus one key
    "sr1_h16": (1, 16, 16, 35, 35, 2405, 1.0),       # sr = 1, 16 heads
    "d8": (1, 4, 8, 256, 4, 2406, 1.0),
    "d32": (1, 2, 32, 100, 33, 2407, 1.0),
    "m5000": (1, 1, 16, 64, 5000, 2408, 1.0),        # more keys than LDS holds: the streaming path
    "level3": (2, 4, 16, 4096, 256, 2409, 1.0),      # the workload's level 3
    "hot": (1, 2, 16, 200, 70, 2410, 8.0),           # max |scale * logit| >= 100: exp overflows without a maximum
}


def core_inputs(name):
    """(q [B,A,N], k [B,A,M], v [B,A,M], go [B,A,N]) float32, and (heads, scale)"""
    b, heads, d, n, m, seed, gain = CORE_CASES[name]
    rng = np.random.default_rng(seed)
    a = heads * d
    q = _f32(rng.standard_normal((b, a, n)) * gain)
    k = _f32(rng.standard_normal((b, a, m)) * gain)
    v = _f32(rng.standard_normal((b, a, m)))
    go = _f32(rng.standard_normal((b, a, n)))
    return q, k, v, go, heads, float(d) ** -0.5


def sra_f64(q, k, v, heads, scale, go=None):
    """float64 restatement of the core.  q [B,A,N], k, v [B,A,M] -> dict(o, lse, zmax (max |scale * logit|), and dq, dk, dv if go)"""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    b, a, n = q.shape
    m, d = k.shape[2], a // heads
    qh, kh, vh = q.reshape(b, heads, d, n), k.reshape(b, heads, d, m), v.reshape(b, heads, d, m)
    o = np.empty((b, heads, d, n))
    lse = np.empty((b, heads, n))
    out = {"zmax": 0.0}
    if go is not None:
        gh = np.asarray(go, np.float64).reshape(b, heads, d, n)
        dq, dk, dv = np.empty_like(qh), np.empty_like(kh), np.empty_like(vh)
    for bb in range(b):
        for h in range(heads):
            z = scale * (qh[bb, h].T @ kh[bb, h])                  # [N, M]
            out["zmax"] = max(out["zmax"], float(np.abs(z).max()))
            zm = z.max(axis=1, keepdims=True)
            e = np.exp(z - zm)
            l = e.sum(axis=1, keepdims=True)
            p = e / l
            lse[bb, h] = (zm + np.log(l))[:, 0]
            o[bb, h] = vh[bb, h] @ p.T                             # [d, N]
            if go is not None:
                g = gh[bb, h]                                      # [d, N]
                dv[bb, h] = g @ p                                  # dv = go P
                dp = g.T @ vh[bb, h]                               # dP = go^T v      [N, M]
                dd = (g * o[bb, h]).sum(axis=0)[:, None]           # D_i = go_i . o_i
                ds = p * (dp - dd)                                 # dS = P o (dP - D)
                dq[bb, h] = scale * (kh[bb, h] @ ds.T)             # dq = scale k dS^T
                dk[bb, h] = scale * (qh[bb, h] @ ds)               # dk = scale q dS
    out["o"], out["lse"] = o.reshape(b, a, n), lse
    if go is not None:
        out["dq"], out["dk"], out["dv"] = dq.reshape(b, a, n), dk.reshape(b, a, m), dv.reshape(b, a, m)
    return out


# ------------------------------------------------------------------ float64 building blocks (forward, and backward by explicit formulas)
def conv1x1_fwd(x, w, b=None):
    y = np.einsum("oc,nchw->nohw", w[:, :, 0, 0], x)
    return y if b is None else y + b[None, :, None, None]


def conv1x1_bwd(x, w, gy):
    """(dx, dw, db)"""
    return (np.einsum("oc,nohw->nchw", w[:, :, 0, 0], gy), np.einsum("nohw,nchw->oc", gy, x)[:, :, None, None], gy.sum(axis=(0, 2, 3)))


def patchconv_fwd(x, w, b=None):
    """depth-wise conv, kernel == stride == s, padding 0: x [N,C,H,W], w [C,1,s,s] -> [N,C,H//s,W//s]"""
    n, c, h, wd = x.shape
    s = w.shape[2]
    oh, ow = h // s, wd // s
    y = np.einsum("ncisjt,cst->ncij", x[:, :, :oh * s, :ow * s].reshape(n, c, oh, s, ow, s), w[:, 0])
    return y if b is None else y + b[None, :, None, None]


def patchconv_bwd(x, w, gy):
    """(dx, dw, db); the rows and columns of dx beyond floor(H / s) s, floor(W / s) s are exactly 0"""
    n, c, h, wd = x.shape
    s = w.shape[2]
    oh, ow = h // s, wd // s
    dx = np.zeros_like(x)
    dx[:, :, :oh * s, :ow * s] = np.einsum("ncij,cst->ncisjt", gy, w[:, 0]).reshape(n, c, oh * s, ow * s)
    dw = np.einsum("ncij,ncisjt->cst", gy, x[:, :, :oh * s, :ow * s].reshape(n, c, oh, s, ow, s))[:, None]
    return dx, dw, gy.sum(axis=(0, 2, 3))


def avgpool_fwd(x, s):
    c = x.shape[1]
    return patchconv_fwd(x, np.full((c, 1, s, s), 1.0 / (s * s)))


def avgpool_bwd(x, s, gy):
    c = x.shape[1]
    return patchconv_bwd(x, np.full((c, 1, s, s), 1.0 / (s * s)), gy)[0]


def dw3_fwd(x, w):
    """depth-wise 3 x 3, reflect padding 1, no bias: w [C,1,3,3]"""
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
    y = np.zeros_like(x)
    for u in range(3):
        for v in range(3):
            y += w[None, :, 0, u, v, None, None] * xp[:, :, u:u + h, v:v + wd]
    return y


def dw3_bwd(x, w, gy):
    """(dx, dw)"""
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
    gp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for u in range(3):
        for v in range(3):
            gp[:, :, u:u + h, v:v + wd] += w[None, :, 0, u, v, None, None] * gy
            dw[:, 0, u, v] = (gy * xp[:, :, u:u + h, v:v + wd]).sum(axis=(0, 2, 3))
    # the adjoint of the reflect padding: padded row 0 is row 1, padded row h + 1 is row h - 2 (columns alike)
    gp[:, :, 2] += gp[:, :, 0]
    gp[:, :, h - 1] += gp[:, :, h + 1]
    gp = gp[:, :, 1:h + 1]
    gp[:, :, :, 2] += gp[:, :, :, 0]
    gp[:, :, :, wd - 1] += gp[:, :, :, wd + 1]
    return gp[:, :, :, 1:wd + 1].copy(), dw


def relu6_fwd(z):
    return np.clip(z, 0.0, 6.0)


def relu6_bwd(y, gy):
    return gy * ((y > 0.0) & (y < 6.0))


def bn_train_fwd(x, gamma, beta, eps=1e-5):
    """nn.BatchNorm2d in train mode: batch statistics, biased variance.  Returns (y, cache)"""
    mean = x.mean(axis=(0, 2, 3), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(0, 2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    return xh * gamma[None, :, None, None] + beta[None, :, None, None], (xh, rstd)


def bn_train_bwd(cache, gamma, gy):
    """(dx, dgamma, dbeta)"""
    xh, rstd = cache
    dxh = gy * gamma[None, :, None, None]
    dx = rstd * (dxh - dxh.mean(axis=(0, 2, 3), keepdims=True) - xh * (dxh * xh).mean(axis=(0, 2, 3), keepdims=True))
    return dx, (gy * xh).sum(axis=(0, 2, 3)), gy.sum(axis=(0, 2, 3))


def layernorm_fwd(x, weight=None, bias=None, eps=1e-6):
    """channel LayerNorm (reference core/block.py:489-500, normalized_dim=(1,)): weight, bias [C,1,1] or None.  Returns (y, cache)"""
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + eps)
    xh = (x - mean) * rstd
    y = xh if weight is None else xh * weight[None]
    return (y if bias is None else y + bias[None]), (xh, rstd)


def layernorm_bwd(cache, weight, gy):
    """(dx, dweight [C,1,1], dbias [C,1,1])"""
    xh, rstd = cache
    gw = gy if weight is None else gy * weight[None]
    dx = rstd * (gw - gw.mean(axis=1, keepdims=True) - xh * (gw * xh).mean(axis=1, keepdims=True))
    return dx, (gy * xh).sum(axis=(0, 2, 3))[:, None, None], gy.sum(axis=(0, 2, 3))[:, None, None]


def join_fwd(a, b, ls=None, rs=None, relu6=False):
    """y = act(ls[c] a + rs[c] b)"""
    z = (a if ls is None else ls[None, :, None, None] * a) + (b if rs is None else rs[None, :, None, None] * b)
    return relu6_fwd(z) if relu6 else z


def join_bwd(a, b, ls, rs, y, gy, relu6=False):
    """(da, db, dls, drs); the ReLU6 mask is taken from y"""
    gm = relu6_bwd(y, gy) if relu6 else gy
    da = gm if ls is None else ls[None, :, None, None] * gm
    db = gm if rs is None else rs[None, :, None, None] * gm
    return da, db, (None if ls is None else (gm * a).sum(axis=(0, 2, 3))), (None if rs is None else (gm * b).sum(axis=(0, 2, 3)))


# ------------------------------------------------------------------ Attention (reference core/block.py:355-434)
# name -> (in_ch, out_ch, input shape, constructor keywords, seed)
ATTN_CASES = {
    "a16": (16, 16, (1, 16, 20, 37), {}, 2421),                        # sr 16, M = 2, ragged
    "a32": (32, 32, (2, 32, 16, 24), {}, 2422),                        # sr 8, M = 6
    "a64_48": (64, 48, (1, 64, 9, 13), {}, 2423),                      # sr 4, M = 6, out_ch != in_ch
    "a128": (128, 128, (1, 128, 6, 10), {}, 2424),                     # sr 2, M = 15
    "a256": (256, 256, (1, 256, 5, 7), {}, 2425),                      # sr 1: k and v from x itself, 16 heads
    "a48_sr5": (48, 48, (1, 48, 11, 12), {"sr_ratio": 5}, 2426),       # sr 5, M = 4
    "a32_h4": (32, 32, (1, 32, 12, 17), {"num_heads": 4}, 2427),       # d = 8
    "a40": (40, 40, (1, 40, 10, 17), {}, 2428),                        # d = 20: outside the kernels, the stock composition
    "a32_avg": (32, 32, (1, 32, 16, 24), {"down_mode": "avgpool"}, 2429),
}


def attn_geometry(in_ch, kw):
    heads = kw.get("num_heads") or in_ch // 16
    d = in_ch // heads
    sr = kw.get("sr_ratio") or 16 // (in_ch // 16)
    return heads, d, heads * d, sr, kw.get("down_mode", "stride")


def attn_param_shapes(in_ch, out_ch, kw, prefix=""):
    heads, d, a, sr, down = attn_geometry(in_ch, kw)
    shapes = {prefix + "q.layers.0.weight": (a, in_ch, 1, 1), prefix + "k.layers.0.weight": (a, in_ch, 1, 1),
              prefix + "v.layers.0.weight": (a, in_ch, 1, 1), prefix + "proj.layers.0.weight": (out_ch, a, 1, 1)}
    if down == "stride":
        shapes[prefix + "pool.layers.0.weight"] = (in_ch, 1, sr, sr)
    return shapes


def make_params(shapes, seed):
    """float32 parameters for a dict key -> shape: conv weights are normal / sqrt(fan-in); norm weights and Scale factors sit near their
    initial value, norm biases near 0"""
    rng = np.random.default_rng(seed)
    out = {}
    for key in sorted(shapes):
        shape = shapes[key]
        if len(shape) == 4:
            out[key] = _f32(rng.standard_normal(shape) / np.sqrt(shape[1] * shape[2] * shape[3]))
        elif key.endswith("bias"):
            out[key] = _f32(0.1 * rng.standard_normal(shape))
        else:
            out[key] = _f32(1.0 + 0.1 * rng.standard_normal(shape))
    return out


def attn_case(name):
    """(x, upstream, params, (in_ch, out_ch, kw)) of an Attention case"""
    in_ch, out_ch, shape, kw, seed = ATTN_CASES[name]
    rng = np.random.default_rng(seed)
    x = _f32(rng.standard_normal(shape))
    g = _f32(rng.standard_normal((shape[0], out_ch) + shape[2:]))
    return x, g, make_params(attn_param_shapes(in_ch, out_ch, kw), seed + 100), (in_ch, out_ch, kw)


def attention_f64(x, params, in_ch, out_ch, kw, g=None, prefix=""):
    """Attention.forward and, with g, its backward: dict(y, dx, and one gradient per parameter key)"""
    heads, d, a, sr, down = attn_geometry(in_ch, kw)
    x = np.asarray(x, np.float64)
    P = {k[len(prefix):]: np.asarray(v, np.float64) for k, v in params.items() if k.startswith(prefix)}
    n, _, h, w = x.shape
    if h < sr or w < sr:
        raise ValueError("the input is smaller than sr_ratio")
    wq, wk, wv, wp = (P[f"{t}.layers.0.weight"] for t in ("q", "k", "v", "proj"))
    q = conv1x1_fwd(x, wq)
    if sr > 1:
        xp = patchconv_fwd(x, P["pool.layers.0.weight"]) if down == "stride" else avgpool_fwd(x, sr)
    else:
        xp = x
    k, v = conv1x1_fwd(xp, wk), conv1x1_fwd(xp, wv)
    m = xp.shape[2] * xp.shape[3]
    scale = float(d) ** -0.5
    go = None
    if g is not None:
        g = np.asarray(g, np.float64)
    core = sra_f64(q.reshape(n, a, h * w), k.reshape(n, a, m), v.reshape(n, a, m), heads, scale)
    o = core["o"].reshape(n, a, h, w)
    out = {"y": conv1x1_fwd(o, wp)}
    if g is None:
        return out
    go, dwp, _ = conv1x1_bwd(o, wp, g)
    core = sra_f64(q.reshape(n, a, h * w), k.reshape(n, a, m), v.reshape(n, a, m), heads, scale, go.reshape(n, a, h * w))
    dx, dwq, _ = conv1x1_bwd(x, wq, core["dq"].reshape(q.shape))
    dxk, dwk, _ = conv1x1_bwd(xp, wk, core["dk"].reshape(k.shape))
    dxv, dwv, _ = conv1x1_bwd(xp, wv, core["dv"].reshape(v.shape))
    dxp = dxk + dxv
    if sr > 1:
        if down == "stride":
            dxa, dwpool, _ = patchconv_bwd(x, P["pool.layers.0.weight"], dxp)
            out[prefix + "pool.layers.0.weight"] = dwpool
        else:
            dxa = avgpool_bwd(x, sr, dxp)
        dx = dx + dxa
    else:
        dx = dx + dxp
    out["dx"] = dx
    out[prefix + "q.layers.0.weight"], out[prefix + "k.layers.0.weight"] = dwq, dwk
    out[prefix + "v.layers.0.weight"], out[prefix + "proj.layers.0.weight"] = dwv, dwp
    return out


# ------------------------------------------------------------------ MetaFormerBlock with an Attention mixer (reference core/block.py:503-540, :603-617)
# name -> (in_ch, out_ch, input shape, norm ('bn' | 'ln'), ReLU6 at the joins, layer_scale, res_scale, seed)
BLOCK_CASES = {
    "transformer32": (32, 32, (2, 32, 16, 24), "bn", True, None, None, 2441),      # TransformerBlock(32, 32), train mode
    "metaformer16": (16, 16, (1, 16, 20, 37), "ln", False, 1e-2, 1.0, 2442),       # MetaFormerBlock(16, 16, token_mixer=Attention, layer_scale=1e-2, res_scale=1.0)
}


def block_param_shapes(name):
    in_ch, out_ch, _, norm, _, ls, rs, _ = BLOCK_CASES[name]
    shapes = attn_param_shapes(in_ch, out_ch, {}, "token_mixer.")
    hid = out_ch * 4
    shapes.update({"ffn.layers.0.layers.0.weight": (hid, out_ch, 1, 1), "ffn.layers.1.layers.0.weight": (hid, 1, 3, 3),
                   "ffn.layers.2.layers.0.weight": (out_ch, hid, 1, 1)})
    for i, c in ((1, in_ch), (2, out_ch)):
        if norm == "bn":
            shapes[f"norm{i}.weight"], shapes[f"norm{i}.bias"] = (c, ), (c, )
        else:
            shapes[f"norm{i}.weight"] = (c, 1, 1)
        if ls:
            shapes[f"layer_scale{i}.scale"] = (out_ch, )
        if rs:
            shapes[f"res_scale{i}.scale"] = (out_ch, )
    return shapes


def block_case(name):
    """(x, upstream, params) of a block case; Scale factors are their initial value times a factor near 1"""
    in_ch, out_ch, shape, _, _, ls, rs, seed = BLOCK_CASES[name]
    rng = np.random.default_rng(seed)
    x = _f32(rng.standard_normal(shape))
    g = _f32(rng.standard_normal((shape[0], out_ch) + shape[2:]))
    params = make_params(block_param_shapes(name), seed + 100)
    for key in params:
        if key.startswith("layer_scale"):
            params[key] = _f32(params[key] * ls)
        elif key.startswith("res_scale"):
            params[key] = _f32(params[key] * rs)
    return x, g, params


def ffn_f64(x, P, g=None):
    """FFN (reference core/block.py:437-457) without norms and biases: 1x1 -> ReLU6 -> depth-wise 3x3 (reflect) -> ReLU6 -> 1x1"""
    w0, w1, w2 = (P[f"ffn.layers.{i}.layers.0.weight"] for i in range(3))
    y0 = relu6_fwd(conv1x1_fwd(x, w0))
    y1 = relu6_fwd(dw3_fwd(y0, w1))
    y = conv1x1_fwd(y1, w2)
    if g is None:
        return y, None
    g1, dw2, _ = conv1x1_bwd(y1, w2, g)
    g0, dw1 = dw3_bwd(y0, w1, relu6_bwd(y1, g1))
    dx, dw0, _ = conv1x1_bwd(x, w0, relu6_bwd(y0, g0))
    return y, (dx, {"ffn.layers.0.layers.0.weight": dw0, "ffn.layers.1.layers.0.weight": dw1, "ffn.layers.2.layers.0.weight": dw2})


def block_f64(name, x, params, g=None):
    """the block's forward (train mode) and, with g, its backward: dict(y, dx, and one gradient per parameter key)"""
    in_ch, out_ch, _, norm, relu6, ls, rs, _ = BLOCK_CASES[name]
    x = np.asarray(x, np.float64)
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}

    def norm_fwd(i, t):
        if norm == "bn":
            return bn_train_fwd(t, P[f"norm{i}.weight"], P[f"norm{i}.bias"])
        return layernorm_fwd(t, P[f"norm{i}.weight"])

    def norm_bwd(i, cache, gt, grads):
        if norm == "bn":
            dt, grads[f"norm{i}.weight"], grads[f"norm{i}.bias"] = bn_train_bwd(cache, P[f"norm{i}.weight"], gt)
        else:
            dt, grads[f"norm{i}.weight"], _ = layernorm_bwd(cache, P[f"norm{i}.weight"], gt)
        return dt

    sc = lambda kind, i: P.get(f"{kind}_scale{i}.scale")
    n1, c1 = norm_fwd(1, x)
    mix = attention_f64(n1, P, in_ch, out_ch, {}, prefix="token_mixer.")["y"]
    y1 = join_fwd(mix, x, sc("layer", 1), sc("res", 1), relu6)
    n2, c2 = norm_fwd(2, y1)
    f, _ = ffn_f64(n2, P)
    y2 = join_fwd(f, y1, sc("layer", 2), sc("res", 2), relu6)
    out = {"y": y2}
    if g is None:
        return out
    g = np.asarray(g, np.float64)
    df, dy1, dls2, drs2 = join_bwd(f, y1, sc("layer", 2), sc("res", 2), y2, g, relu6)
    _, (dn2, fg) = ffn_f64(n2, P, df)
    out.update(fg)
    dy1 = dy1 + norm_bwd(2, c2, dn2, out)
    dmix, dx, dls1, drs1 = join_bwd(mix, x, sc("layer", 1), sc("res", 1), y1, dy1, relu6)
    att = attention_f64(n1, P, in_ch, out_ch, {}, g=dmix, prefix="token_mixer.")
    for k, v in att.items():
        if k.startswith("token_mixer."):
            out[k] = v
    out["dx"] = dx + norm_bwd(1, c1, att["dx"], out)
    for key, val in (("layer_scale1.scale", dls1), ("res_scale1.scale", drs1), ("layer_scale2.scale", dls2), ("res_scale2.scale", drs2)):
        if val is not None:
            out[key] = val
    return out


# ------------------------------------------------------------------ the small kernels
PATCH_S = (2, 5, 8, 16)


def patch_case(s, bias, seed=2460):
    """x [2,6,3s+1,2s+3], w [6,1,s,s], bias [6] or None, upstream [2,6,(3s+1)//s,(2s+3)//s]"""
    rng = np.random.default_rng(seed + s)
    x = _f32(rng.standard_normal((2, 6, 3 * s + 1, 2 * s + 3)))
    w = _f32(rng.standard_normal((6, 1, s, s)) / s)
    b = _f32(rng.standard_normal(6)) if bias else None
    return x, w, b, _f32(rng.standard_normal((2, 6, (3 * s + 1) // s, (2 * s + 3) // s)))


def patch_f64(x, w, b, g, relu6):
    """ConvLayer(6, 6, ksize=s, stride=s, padding=0, groups=6, bias=..., act=ReLU6 | None): dict(y, dx, dw, db)"""
    x, w, g = (np.asarray(t, np.float64) for t in (x, w, g))
    b = None if b is None else np.asarray(b, np.float64)
    z = patchconv_fwd(x, w, b)
    y = relu6_fwd(z) if relu6 else z
    dx, dw, db = patchconv_bwd(x, w, relu6_bwd(y, g) if relu6 else g)
    return {"y": y, "dx": dx, "dw": dw, "db": db}


LN_C = (1, 7, 16, 256)


def ln_case(c, seed=2480):
    """x [2,c,5,9], weight, bias [c,1,1], upstream"""
    rng = np.random.default_rng(seed + c)
    return (_f32(rng.standard_normal((2, c, 5, 9)) * 2.0 + 0.5), _f32(1.0 + 0.3 * rng.standard_normal((c, 1, 1))), _f32(0.3 * rng.standard_normal((c, 1, 1))),
            _f32(rng.standard_normal((2, c, 5, 9))))


def ln_f64(x, weight, bias, g, eps=1e-6):
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    weight = None if weight is None else np.asarray(weight, np.float64)
    bias = None if bias is None else np.asarray(bias, np.float64)
    y, cache = layernorm_fwd(x, weight, bias, eps)
    dx, dw, db = layernorm_bwd(cache, weight, g)
    return {"y": y, "dx": dx, "dw": dw, "db": db}


def join_case(seed=2490):
    """a, b [2,5,7,9] (scaled so that ReLU6 clips at both ends), ls, rs [5], upstream"""
    rng = np.random.default_rng(seed)
    shape = (2, 5, 7, 9)
    return (_f32(rng.standard_normal(shape) * 3.0), _f32(rng.standard_normal(shape) * 3.0), _f32(1.0 + 0.5 * rng.standard_normal(5)),
            _f32(1.0 + 0.5 * rng.standard_normal(5)), _f32(rng.standard_normal(shape)))


def join_f64(a, b, ls, rs, g, relu6):
    a, b, g = (np.asarray(t, np.float64) for t in (a, b, g))
    ls = None if ls is None else np.asarray(ls, np.float64)
    rs = None if rs is None else np.asarray(rs, np.float64)
    y = join_fwd(a, b, ls, rs, relu6)
    da, db, dls, drs = join_bwd(a, b, ls, rs, y, g, relu6)
    return {"y": y, "da": da, "db": db, "dls": dls, "drs": drs}
