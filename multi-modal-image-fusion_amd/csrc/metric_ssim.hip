// The metric-side SSIM and MS-SSIM of the reference's core/metric.py:290-403 for every window 1..11, with and without reflect padding,
// as per-pixel maps and per-sample sums: calc_ssim(win_size, use_padding, size_average, full) and calc_msssim(win_size, use_padding).
// Forward only, two images, the window a run-time value:
//   k      = min(win_size, h, w), even k included; sigma 1.5 for every k (the loss side's 0.15 (k - 1) rule does not apply here)
//   window = the reference's create_window: taps exp(.) in double -> fp32, divided by torch's fp32 sum of the taps; the 2-D weight is
//            the fp32 PRODUCT of two taps (torch.mm of [k,1] x [1,k]), so the k x k sum below uses those k^2 fp32 values, not a
//            separable pass with the unrounded products
//   map    = (h - k + 1) x (w - k + 1) without padding; with padding every pass sees the image reflect-padded by p = k / 2 (torch
//            'reflect': the edge pixel is not repeated): (h + 2p - k + 1) x (w + 2p - k + 1), i.e. h x w for odd and (h + 1) x (w + 1)
//            for even k.  The padding is index arithmetic in the tile loader.
//   pixel  = :331-355: both variances clamped at 0, the covariance not; cs = v1 / v2, ssim = m1 v1 / (m2 v2)
// The five window moments and the pixel arithmetic run in fp64 on the fp32 pixels: this is evaluation code (one launch per call, the
// k^2 x 5 fp64 FMAs per pixel are a few microseconds at full size), and in fp64 the variance of a near-flat image (200 + U(0, 0.5):
// E[x^2] - mu^2 cancels five digits) is as good as the reference run on float64 tensors, which is what the tests hold it to.  The maps
// are rounded to fp32 once, at the store; the sums take the fp64 values.
// A 16 x 16 map tile per block with its (16 + k - 1)^2 halo in LDS; fp64 block sums, then one block per sample adds its tiles in a
// fixed order: a sample's sums do not depend on the batch it is in.  No atomics.
#include <math.h>

#include "common.hpp"
#include "ssim_common.hpp"

namespace mmif {

constexpr int MS_T = 16;      // map tile edge
constexpr int MS_KMAX = SSIM_KMAX;   // largest window
constexpr int MS_LIN = MS_T + MS_KMAX - 1;

struct MetricWin {
    float w[MS_KMAX * MS_KMAX];   // w[i * k + j] = fp32(t_i * t_j)
};

// the reference's create_window on the taps of _gaussian_kernel(k, 1.5) (ssim_taps of ssim_common.hpp): win[k][k], the fp32 products;
// tests/test_ssim_metric_oracle_cpu.py pins every k = 1..11 bit for bit.
static void metric_window(const SsimTaps& taps, int k, float* win) {
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) win[i * k + j] = taps.t[i] * taps.t[j];
}

// one 16 x 16 tile of the maps of sample blockIdx.x / tiles.  P = 0 without padding, k / 2 with.  ssim_map, cs_map [n][Hm][Wm] and
// partial [n][tiles][2] (sum ssim, sum cs of the tile) are each optional.
template <typename TIN>
__global__ __launch_bounds__(256) void metric_ssim_kernel(const TIN* __restrict__ x1, const TIN* __restrict__ x2, int H, int W, int Hm, int Wm,
                                                          int k, int P, MetricWin win, double C1, double C2, float* __restrict__ ssim_map,
                                                          float* __restrict__ cs_map, double* __restrict__ partial, int tiles_x, int tiles) {
    __shared__ double in[2][MS_LIN][MS_LIN + 1];
    __shared__ double red[2][256];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int mx0 = (t % tiles_x) * MS_T, my0 = (t / tiles_x) * MS_T;
    const long long ibase = (long long)b * H * W;
    const int lin = MS_T + k - 1;
    const int Hp = H + 2 * P, Wp = W + 2 * P;   // the extent the window pass sees
    for (int e = tid; e < lin * lin; e += 256) {
        const int py = e / lin, px = e % lin;
        const int Y = my0 + py, X = mx0 + px;
        const bool ok = (Y < Hp) && (X < Wp);
        // padded row Y mirrors image row reflect(Y - P); P <= k / 2 < H, W (k <= H, W), so one reflection lands inside
        const int y = ok ? min(max(reflect_idx(Y - P, H), 0), H - 1) : 0;
        const int x = ok ? min(max(reflect_idx(X - P, W), 0), W - 1) : 0;
        const long long i = ibase + (long long)y * W + x;
        in[0][py][px] = ok ? (double)x1[i] : 0.0;
        in[1][py][px] = ok ? (double)x2[i] : 0.0;
    }
    __syncthreads();
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) {
            const double wv = (double)win.w[i * k + j];
            const double a = in[0][ty + i][tx + j], c = in[1][ty + i][tx + j];
            mu1 = fma(wv, a, mu1);
            mu2 = fma(wv, c, mu2);
            e11 = fma(wv, a * a, e11);
            e22 = fma(wv, c * c, e22);
            e12 = fma(wv, a * c, e12);
        }
    }
    const int my = my0 + ty, mx = mx0 + tx;
    const bool valid = (my < Hm) && (mx < Wm);
    double ssim = 0.0, cs = 0.0;
    if (valid) {
        const double s1 = fmax(e11 - mu1 * mu1, 0.0), s2 = fmax(e22 - mu2 * mu2, 0.0);
        const double s12 = e12 - mu1 * mu2;
        const double m1 = 2.0 * (mu1 * mu2) + C1, m2 = mu1 * mu1 + mu2 * mu2 + C1;
        const double v1 = 2.0 * s12 + C2, v2 = s1 + s2 + C2;
        cs = v1 / v2;
        ssim = (m1 * v1) / (m2 * v2);
        const long long o = ((long long)b * Hm + my) * Wm + mx;
        if (ssim_map != nullptr) ssim_map[o] = (float)ssim;
        if (cs_map != nullptr) cs_map[o] = (float)cs;
    }
    if (partial == nullptr) return;
    red[0][tid] = ssim;
    red[1][tid] = cs;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        partial[2 * (long long)blockIdx.x] = red[0][0];
        partial[2 * (long long)blockIdx.x + 1] = red[1][0];
    }
}

// sample b = blockIdx.x: o_ssim[b * stride] = scale * sum_t partial[b][t][0], o_cs likewise from [1] (each optional); with dup != 0
// the value is stored at [b * stride + dup] as well.  Thread i adds tiles i, i + 256, ... in order, then a fixed tree.
__global__ __launch_bounds__(256) void metric_ssim_sum_kernel(const double* __restrict__ partial, int tiles, double scale,
                                                              double* __restrict__ o_ssim, double* __restrict__ o_cs, int stride, long long dup) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const double* p = partial + 2 * (long long)b * tiles;
    double s = 0.0, c = 0.0;
    for (int t = tid; t < tiles; t += 256) {
        s += p[2 * (long long)t];
        c += p[2 * (long long)t + 1];
    }
    red[0][tid] = s;
    red[1][tid] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const long long o = (long long)b * stride;
    if (o_ssim != nullptr) {
        o_ssim[o] = red[0][0] * scale;
        if (dup != 0) o_ssim[o + dup] = red[0][0] * scale;
    }
    if (o_cs != nullptr) {
        o_cs[o] = red[1][0] * scale;
        if (dup != 0) o_cs[o + dup] = red[1][0] * scale;
    }
}

struct MapGeom {
    int k, p, hm, wm, tiles_x, tiles;
};
static MapGeom map_geom(int h, int w, int win_size, int use_padding) {
    MapGeom g;
    g.k = win_size < h ? win_size : h;
    g.k = g.k < w ? g.k : w;
    g.p = use_padding ? g.k / 2 : 0;
    g.hm = ssim_map_extent(h, g.k, use_padding);
    g.wm = ssim_map_extent(w, g.k, use_padding);
    g.tiles_x = cdiv(g.wm, MS_T);
    g.tiles = g.tiles_x * cdiv(g.hm, MS_T);
    return g;
}

// the window pass of one pair of n images; partial (optional) gets [n][tiles][2]
template <typename TIN>
static int run_maps(const TIN* x1, const TIN* x2, int n, int h, int w, const MapGeom& g, double data_range, float* ssim_map, float* cs_map,
                    double* partial, hipStream_t st) {
    MetricWin win;
    memset(&win, 0, sizeof(win));
    metric_window(ssim_taps(g.k, 1.5), g.k, win.w);
    const SsimConsts<double> c = ssim_consts(data_range);
    hipLaunchKernelGGL((metric_ssim_kernel<TIN>), dim3((unsigned)n * g.tiles), dim3(256), 0, st, x1, x2, h, w, g.hm, g.wm, g.k, g.p, win, c.C1, c.C2,
                       ssim_map, cs_map, partial, g.tiles_x, g.tiles);
    return check_launch("metric_ssim");
}

static bool grid_fits(int n, const MapGeom& g) { return (long long)n * g.tiles < 0x7fffffffll; }

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace mmif

using namespace mmif;

extern "C" int mmif_metric_ssim_window(int32_t win_size, float* taps, float* window) {
    MMIF_REQUIRE(win_size >= 1 && win_size <= MS_KMAX, "metric_ssim_window: win_size must be 1..11 (got %d)", win_size);
    MMIF_REQUIRE(taps && window, "metric_ssim_window: NULL argument");
    const SsimTaps t = ssim_taps(win_size, 1.5);
    for (int i = 0; i < win_size; ++i) taps[i] = t.t[i];
    metric_window(t, win_size, window);
    return MMIF_OK;
}

extern "C" size_t mmif_metric_ssim_maps_workspace(int32_t n, int32_t h, int32_t w, int32_t win_size, int32_t use_padding) {
    if (n < 1 || h < 1 || w < 1 || win_size < 1) return 0;
    const MapGeom g = map_geom(h, w, win_size, use_padding);
    if (g.k > MS_KMAX || !grid_fits(n, g)) return 0;
    return align256(2 * (size_t)n * g.tiles * sizeof(double));
}

extern "C" int mmif_metric_ssim_maps(const float* img1, const float* img2, int32_t n, int32_t h, int32_t w, int32_t win_size,
                                     int32_t use_padding, double data_range, float* ssim_map, float* cs_map, double* sums, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(img1 && img2, "metric_ssim_maps: NULL image");
    MMIF_REQUIRE(n >= 1 && h >= 1 && w >= 1, "metric_ssim_maps: empty batch or image (n=%d, %dx%d)", n, h, w);
    MMIF_REQUIRE(win_size >= 1, "metric_ssim_maps: win_size must be at least 1 (got %d)", win_size);
    const MapGeom g = map_geom(h, w, win_size, use_padding);
    MMIF_REQUIRE(g.k <= MS_KMAX, "metric_ssim_maps: window min(win_size, h, w) = %d, the kernel covers windows up to 11", g.k);
    MMIF_REQUIRE(ssim_map || cs_map || sums, "metric_ssim_maps: no output requested (ssim_map, cs_map and sums are all NULL)");
    MMIF_REQUIRE(grid_fits(n, g), "metric_ssim_maps: too many tiles (n=%d, %dx%d)", n, h, w);
    if (sums != nullptr && (workspace == nullptr || workspace_bytes < mmif_metric_ssim_maps_workspace(n, h, w, win_size, use_padding))) {
        set_error("metric_ssim_maps: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double* partial = sums != nullptr ? (double*)workspace : nullptr;
    if (int rc = run_maps<float>(img1, img2, n, h, w, g, data_range, ssim_map, cs_map, partial, st)) return rc;
    if (sums != nullptr) {
        hipLaunchKernelGGL(metric_ssim_sum_kernel, dim3(n), dim3(256), 0, st, partial, g.tiles, 1.0, sums, sums + 1, 2, 0ll);
        return check_launch("metric_ssim sums");
    }
    return MMIF_OK;
}

// workspace: [partial: 2 n tiles(level 0) doubles | levels 1..4: three fp64 images each]
extern "C" size_t mmif_metric_msssim_any_workspace(int32_t n, int32_t h, int32_t w) {
    if (n < 1 || h < 9 || w < 9) return 0;
    size_t bytes = align256(2 * (size_t)n * cdiv(h + 1, MS_T) * cdiv(w + 1, MS_T) * sizeof(double));   // (h + 1) x (w + 1): padded even window
    const SsimPyramid py = ssim_pyramid(h, w);
    for (int l = 1; l < SSIM_LEVELS; ++l) bytes += 3 * align256((size_t)n * py.pixels(l) * sizeof(double));
    return bytes;
}

// one level of one pair: the window pass, then the per-sample means into out rows
template <typename TIN>
static int msssim_level(const TIN* x, const TIN* f, int n, int h, int w, int win_size, int use_padding, double data_range, double* partial,
                        double* o_ssim, double* o_cs, long long dup, hipStream_t st) {
    const MapGeom g = map_geom(h, w, win_size, use_padding);
    if (int rc = run_maps<TIN>(x, f, n, h, w, g, data_range, nullptr, nullptr, partial, st)) return rc;
    hipLaunchKernelGGL(metric_ssim_sum_kernel, dim3(n), dim3(256), 0, st, partial, g.tiles, 1.0 / ((double)g.hm * (double)g.wm), o_ssim, o_cs, 1, dup);
    return check_launch("metric_msssim_any means");
}

extern "C" int mmif_metric_msssim_any(const float* a, const float* b, const float* f, int32_t n, int32_t h, int32_t w, int32_t win_size,
                                      int32_t use_padding, double data_range, double* out, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    MMIF_REQUIRE(a && f && out, "metric_msssim_any: NULL argument");
    MMIF_REQUIRE(n >= 1, "metric_msssim_any: empty batch (n=%d)", n);
    MMIF_REQUIRE(win_size >= 1, "metric_msssim_any: win_size must be at least 1 (got %d)", win_size);
    MMIF_REQUIRE(h >= 9 && w >= 9, "metric_msssim_any: images must be at least 9x9 (level 3 of a smaller one is 1 px wide and cannot be "
                 "reflect-padded); got %dx%d", h, w);
    const MapGeom g0 = map_geom(h, w, win_size, use_padding);
    MMIF_REQUIRE(g0.k <= MS_KMAX, "metric_msssim_any: window min(win_size, h, w) = %d, the kernel covers windows up to 11", g0.k);
    MMIF_REQUIRE(grid_fits(n, g0), "metric_msssim_any: too many tiles (n=%d, %dx%d)", n, h, w);
    if (workspace == nullptr || workspace_bytes < mmif_metric_msssim_any_workspace(n, h, w)) {
        set_error("metric_msssim_any: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int npairs = b != nullptr ? 2 : 1;
    const long long dup = b != nullptr ? 0 : 6ll * n;   // b == NULL: pair 2 repeats pair 1
    char* wsp = (char*)workspace;
    double* partial = (double*)wsp;
    wsp += align256(2 * (size_t)n * cdiv(h + 1, MS_T) * cdiv(w + 1, MS_T) * sizeof(double));
    const float* src[2] = {a, b};
    // level 0 on the fp32 images: cs -> slot 0, ssim -> slot 5
    for (int p = 0; p < npairs; ++p)
        if (int rc = msssim_level<float>(src[p], f, n, h, w, win_size, use_padding, data_range, partial, out + (p * 6 + 5) * (long long)n,
                                         out + (p * 6 + 0) * (long long)n, dup, st))
            return rc;
    // levels 1..4 on fp64 pyramids (the pooling of fp32 pixels is exact enough in double to be the definition's)
    const SsimPyramid py = ssim_pyramid(h, w);
    const float* const lv0[3] = {a, b, f};
    double* lv[3] = {nullptr, nullptr, nullptr};   // a, b (unused where b == NULL), f of the previous level
    for (int l = 1; l < 5; ++l) {
        double* cur[3];
        for (int q = 0; q < 3; ++q) {
            cur[q] = (double*)wsp;
            wsp += align256((size_t)n * py.pixels(l) * sizeof(double));
        }
        const double* const prev[3] = {lv[0], b != nullptr ? lv[1] : nullptr, lv[2]};
        if (int rc = l == 1 ? avg_pool_pad3(lv0, cur, n, h, w, st, "metric_msssim_any pool")
                            : avg_pool_pad3(prev, cur, n, py.h[l - 1], py.w[l - 1], st, "metric_msssim_any pool"))
            return rc;
        for (int q = 0; q < 3; ++q) lv[q] = cur[q];
        const int hl = py.h[l], wl = py.w[l];
        for (int p = 0; p < npairs; ++p) {
            double* row = out + (p * 6 + l) * (long long)n;
            if (int rc = msssim_level<double>(lv[p], lv[2], n, hl, wl, win_size, use_padding, data_range, partial, l == 4 ? row : nullptr,
                                              l == 4 ? nullptr : row, dup, st))
                return rc;
        }
    }
    return MMIF_OK;
}
