// Glue of the MetaFormer blocks (reference core/block.py:472-540) on plain NCHW fp32 tensors [n][c][hw]:
//   channel LayerNorm   y = (x - mean_c x) / sqrt(var_c x + eps) * weight[c] + bias[c]   per pixel, biased variance, c <= 256
//   residual join       y = act(ls[c] a + rs[c] b), act = none | ReLU6, ls / rs the optional Scale parameters
// Every channel sum (dweight, dbias, dls, drs) runs in two stages: block (channel, one of GLUE_CHUNKS chunks of the channel's n * hw elements)
// -> partials, then the chunks in chunk order.  The chunk count is a constant: no atomics, bit-identical run to run on any device.
#include "common.hpp"

namespace mmif {
namespace {

constexpr int LN_MAXC = 256;
constexpr int GLUE_CHUNKS = 64;

// one thread per pixel; neighbouring threads read neighbouring pixels of one channel plane
__global__ void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y,
                              float* __restrict__ stats, long long total, int c, long long hw, float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long in_ = i / hw, px = i - in_ * hw;
    const float* xp = x + in_ * c * hw + px;
    float m = 0.f;
    for (int ch = 0; ch < c; ++ch) m += xp[(long long)ch * hw];
    m /= (float)c;
    float v = 0.f;
    for (int ch = 0; ch < c; ++ch) {
        const float d = xp[(long long)ch * hw] - m;
        v = fmaf(d, d, v);
    }
    const float rstd = 1.f / sqrtf(v / (float)c + eps);
    stats[2 * i] = m;
    stats[2 * i + 1] = rstd;
    float* yp = y + in_ * c * hw + px;
    for (int ch = 0; ch < c; ++ch) {
        float r = (xp[(long long)ch * hw] - m) * rstd;
        if (w != nullptr) r *= w[ch];
        if (b != nullptr) r += b[ch];
        yp[(long long)ch * hw] = r;
    }
}

// dx = rstd (gw - mean_c gw - xhat mean_c(gw xhat)),  gw = g weight
__global__ void ln_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ stats,
                                 float* __restrict__ dx, long long total, int c, long long hw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long in_ = i / hw, px = i - in_ * hw, base = in_ * c * hw + px;
    const float m = stats[2 * i], rstd = stats[2 * i + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int ch = 0; ch < c; ++ch) {
        const long long a = base + (long long)ch * hw;
        const float gw = w != nullptr ? g[a] * w[ch] : g[a];
        s1 += gw;
        s2 = fmaf(gw, (x[a] - m) * rstd, s2);
    }
    s1 /= (float)c;
    s2 /= (float)c;
    for (int ch = 0; ch < c; ++ch) {
        const long long a = base + (long long)ch * hw;
        const float gw = w != nullptr ? g[a] * w[ch] : g[a];
        dx[a] = rstd * (gw - s1 - (x[a] - m) * rstd * s2);
    }
}

// elements [e0, e1) of channel ch, e = sample * hw + pixel, for block (ch, chunk)
__device__ inline void glue_chunk(long long total, long long& e0, long long& e1) {
    const long long per = ((total + GLUE_CHUNKS - 1) / GLUE_CHUNKS + 255) / 256 * 256;
    e0 = (long long)blockIdx.y * per;
    e1 = e0 + per < total ? e0 + per : total;
}

// stage 1 of dweight / dbias: part[chunk][c][2] = (sum g xhat, sum g) over the chunk
__global__ __launch_bounds__(256) void ln_bwd_affine_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ stats,
                                                            float* __restrict__ part, int n, int c, long long hw) {
    __shared__ float red[16];
    const int ch = blockIdx.x;
    long long e0, e1;
    glue_chunk((long long)n * hw, e0, e1);
    float sw = 0.f, sb = 0.f;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const long long in_ = e / hw, a = (in_ * c + ch) * hw + (e - in_ * hw);
        const float gv = g[a];
        sw = fmaf(gv, (x[a] - stats[2 * e]) * stats[2 * e + 1], sw);
        sb += gv;
    }
    const float tw = block_sum(sw, red);
    const float tb = block_sum(sb, red);
    if (threadIdx.x == 0) {
        float* out = part + ((long long)blockIdx.y * c + ch) * 2;
        out[0] = tw;
        out[1] = tb;
    }
}

// stage 2: out0[c], out1[c] = sum of the chunk partials, in chunk order (either may be NULL)
__global__ void glue_chan_reduce(const float* __restrict__ part, float* __restrict__ out0, float* __restrict__ out1, int c) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    float a = 0.f, b = 0.f;
    for (int k = 0; k < GLUE_CHUNKS; ++k) {
        a += part[((long long)k * c + ch) * 2];
        b += part[((long long)k * c + ch) * 2 + 1];
    }
    if (out0 != nullptr) out0[ch] = a;
    if (out1 != nullptr) out1[ch] = b;
}

__device__ inline float join_act(float z, int act) { return act == 4 ? fminf(fmaxf(z, 0.f), 6.f) : z; }
__device__ inline float join_mask(float y, int act) { return act == 4 ? ((y > 0.f && y < 6.f) ? 1.f : 0.f) : 1.f; }   // ReLU6: zero at and beyond both bounds

__global__ void join_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ ls, const float* __restrict__ rs,
                                float* __restrict__ y, long long total, int c, long long hw, int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)((i / hw) % c);
        const float l = ls != nullptr ? ls[ch] : 1.f, r = rs != nullptr ? rs[ch] : 1.f;
        y[i] = join_act(fmaf(l, a[i], r * b[i]), act);
    }
}

// with Scale parameters, stage 1: da = ls gm, db = rs gm, part[chunk][c][2] = (sum gm a, sum gm b) over the chunk, gm = g [mask from y]
__global__ __launch_bounds__(256) void join_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ ls,
                                                       const float* __restrict__ rs, const float* __restrict__ y, const float* __restrict__ g,
                                                       float* __restrict__ da, float* __restrict__ db, float* __restrict__ part, int n, int c, long long hw,
                                                       int act) {
    __shared__ float red[16];
    const int ch = blockIdx.x;
    const float l = ls != nullptr ? ls[ch] : 1.f, r = rs != nullptr ? rs[ch] : 1.f;
    long long e0, e1;
    glue_chunk((long long)n * hw, e0, e1);
    float sl = 0.f, sr = 0.f;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const long long in_ = e / hw, i = (in_ * c + ch) * hw + (e - in_ * hw);
        const float gm = g[i] * join_mask(y[i], act);
        da[i] = l * gm;
        db[i] = r * gm;
        if (ls != nullptr) sl = fmaf(gm, a[i], sl);
        if (rs != nullptr) sr = fmaf(gm, b[i], sr);
    }
    const float tl = block_sum(sl, red);
    const float tr = block_sum(sr, red);
    if (threadIdx.x == 0) {
        float* out = part + ((long long)blockIdx.y * c + ch) * 2;
        out[0] = tl;
        out[1] = tr;
    }
}

// without Scale parameters there is no channel sum: da = db = g [mask from y], any grid
__global__ void join_bwd_plain_kernel(const float* __restrict__ y, const float* __restrict__ g, float* __restrict__ da, float* __restrict__ db,
                                      long long total, int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float gm = g[i] * join_mask(y[i], act);
        da[i] = gm;
        db[i] = gm;
    }
}

int grid1d(long long total) {
    const long long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 65535 * 16 ? 65535 * 16 : b));
}

int check_plane(const char* what, int n, int c, long long hw) {
    MMIF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535, "%s: bad extent (n %d, c %d, hw %lld)", what, n, c, hw);
    MMIF_REQUIRE((long long)n * c * hw / 256 < 0x7fffffffll, "%s: n * c * hw too large", what);
    return MMIF_OK;
}

}  // namespace
}  // namespace mmif

using namespace mmif;

// stats: fp32 [n][hw][2] = (mean, 1 / sqrt(var + eps)) of every pixel, written by fwd and read by bwd
extern "C" int mmif_layernorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* stats, int32_t n, int32_t c, int64_t hw, float eps,
                                  void* stream) {
    if (int rc = check_plane("layernorm_fwd", n, c, hw)) return rc;
    MMIF_REQUIRE(c <= LN_MAXC, "layernorm_fwd: at most %d channels (got %d)", LN_MAXC, c);
    MMIF_REQUIRE(x != nullptr && y != nullptr && stats != nullptr, "layernorm_fwd: null pointer");
    const long long total = (long long)n * hw;
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, weight, bias, y, stats, total, c, (long long)hw,
                       eps);
    return check_launch("layernorm_fwd");
}

// bytes of the partial channel sums of mmif_layernorm_bwd / mmif_join_bwd
extern "C" size_t mmif_glue_workspace(int32_t c) { return c > 0 ? (size_t)GLUE_CHUNKS * c * 2 * sizeof(float) : 0; }

extern "C" int mmif_layernorm_bwd(const float* x, const float* gy, const float* weight, const float* stats, float* dx, float* dweight, float* dbias, int32_t n,
                                  int32_t c, int64_t hw, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_plane("layernorm_bwd", n, c, hw)) return rc;
    MMIF_REQUIRE(c <= LN_MAXC, "layernorm_bwd: at most %d channels (got %d)", LN_MAXC, c);
    MMIF_REQUIRE(x != nullptr && gy != nullptr && stats != nullptr && dx != nullptr, "layernorm_bwd: null pointer");
    const bool affine = dweight != nullptr || dbias != nullptr;
    if (affine && (workspace == nullptr || workspace_bytes < mmif_glue_workspace(c))) {
        set_error("layernorm_bwd: workspace of %zu bytes, needs %zu", workspace == nullptr ? (size_t)0 : workspace_bytes, mmif_glue_workspace(c));
        return MMIF_EWORKSPACE;
    }
    const long long total = (long long)n * hw;
    hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, gy, weight, stats, dx, total, c, (long long)hw);
    if (int rc = check_launch("layernorm_bwd dx")) return rc;
    if (!affine) return MMIF_OK;
    hipLaunchKernelGGL(ln_bwd_affine_kernel, dim3(c, GLUE_CHUNKS), dim3(256), 0, (hipStream_t)stream, x, gy, stats, (float*)workspace, n, c, (long long)hw);
    if (int rc = check_launch("layernorm_bwd affine")) return rc;
    hipLaunchKernelGGL(glue_chan_reduce, dim3(cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dweight, dbias, c);
    return check_launch("layernorm_bwd affine sum");
}

// act: 0 none, 4 ReLU6 (the codes of mmif_act_fwd)
extern "C" int mmif_join_fwd(const float* a, const float* b, const float* ls, const float* rs, float* y, int32_t n, int32_t c, int64_t hw, int32_t act,
                             void* stream) {
    if (int rc = check_plane("join_fwd", n, c, hw)) return rc;
    MMIF_REQUIRE(act == 0 || act == 4, "join_fwd: act must be 0 (none) or 4 (ReLU6), got %d", act);
    MMIF_REQUIRE(a != nullptr && b != nullptr && y != nullptr, "join_fwd: null pointer");
    const long long total = (long long)n * c * hw;
    hipLaunchKernelGGL(join_fwd_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, a, b, ls, rs, y, total, c, (long long)hw, act);
    return check_launch("join_fwd");
}

extern "C" int mmif_join_bwd(const float* a, const float* b, const float* ls, const float* rs, const float* y, const float* gy, float* da, float* db, float* dls,
                             float* drs, int32_t n, int32_t c, int64_t hw, int32_t act, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_plane("join_bwd", n, c, hw)) return rc;
    MMIF_REQUIRE(act == 0 || act == 4, "join_bwd: act must be 0 (none) or 4 (ReLU6), got %d", act);
    MMIF_REQUIRE(y != nullptr && gy != nullptr && da != nullptr && db != nullptr, "join_bwd: null pointer");
    MMIF_REQUIRE((dls == nullptr || (ls != nullptr && a != nullptr)) && (drs == nullptr || (rs != nullptr && b != nullptr)), "join_bwd: a scale gradient needs its scale and operand");
    if (ls == nullptr && rs == nullptr) {
        const long long total = (long long)n * c * hw;
        hipLaunchKernelGGL(join_bwd_plain_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, y, gy, da, db, total, act);
        return check_launch("join_bwd");
    }
    MMIF_REQUIRE((ls == nullptr || a != nullptr) && (rs == nullptr || b != nullptr), "join_bwd: a scale needs its operand");
    if (workspace == nullptr || workspace_bytes < mmif_glue_workspace(c)) {
        set_error("join_bwd: workspace of %zu bytes, needs %zu", workspace == nullptr ? (size_t)0 : workspace_bytes, mmif_glue_workspace(c));
        return MMIF_EWORKSPACE;
    }
    hipLaunchKernelGGL(join_bwd_kernel, dim3(c, GLUE_CHUNKS), dim3(256), 0, (hipStream_t)stream, a, b, ls, rs, y, gy, da, db, (float*)workspace, n, c,
                       (long long)hw, act);
    if (int rc = check_launch("join_bwd")) return rc;
    hipLaunchKernelGGL(glue_chan_reduce, dim3(cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dls, drs, c);
    return check_launch("join_bwd scale sum");
}
