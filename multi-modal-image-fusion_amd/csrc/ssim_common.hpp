// The building blocks the SSIM kernels share: the 'ssim' loss of the train step (loss.hip), the SSIMLoss modes with and without reflect
// padding (loss_modes.hip) and the metric-side SSIM / MS-SSIM (metric_ssim.hip).  Each of these has its only definition here: the window
// taps, the per-pixel pair terms with their adjoint coefficients, the map extent and the C1 / C2 constants, the level sizes and the
// pooling step of the 5-level pyramid, and the grid of the element-wise kernels.
#pragma once
#include <math.h>

#include "common.hpp"

namespace mmif {

// ------------------------------------------------------------------ window taps
constexpr int SSIM_KMAX = 11;   // largest window

struct SsimTaps {
    float t[SSIM_KMAX];         // taps 0 .. k - 1 of a k-tap window, zeros behind them
};

// The reference's _gaussian_kernel (core/loss.py:24-39, core/metric.py): taps exp(.) in double -> float32, divided by their float32
// sum.  The sum is torch's float32 sum of a short vector: four interleaved partial sums combined pairwise.  For 5, 7, 9 and 11 taps
// that is the correctly rounded sum; for 3 taps at the loss side's sigma it is one ulp above it (golden F20 'msw-ssim_255' shows the
// difference; tests/test_loss_oracle_cpu.py and tests/test_ssim_metric_oracle_cpu.py pin the taps of every k bit for bit).
inline SsimTaps ssim_taps(int k, double sigma) {
    SsimTaps w;
    float g[SSIM_KMAX];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < k; ++i) {
        g[i] = (float)exp(-(double)((i - k / 2) * (i - k / 2)) / (2.0 * sigma * sigma));
        acc[i & 3] += g[i];
    }
    const float fs = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    for (int i = 0; i < SSIM_KMAX; ++i) w.t[i] = i < k ? g[i] / fs : 0.f;
    return w;
}
// the loss side's sigma (core/loss.py:33-39); the metric side takes 1.5 for every k
inline double ssim_loss_sigma(int k) { return k == 11 ? 1.5 : 0.15 * (k - 1); }

// ------------------------------------------------------------------ map extent and constants
// extent of the map of a k-tap window pass over `extent` pixels: valid correlation, or with `padded` the image reflect-padded by k / 2
// on both sides first (the image's own extent for odd k, one more for even k)
__host__ __device__ constexpr int ssim_map_extent(int extent, int k, int padded) { return extent + 2 * (padded ? k / 2 : 0) - k + 1; }
// pixels of that map, as the float the means divide by
inline float ssim_map_count(int h, int w, int k, int padded) { return (float)ssim_map_extent(h, k, padded) * (float)ssim_map_extent(w, k, padded); }

template <typename T>
struct SsimConsts {
    T C1, C2;   // (0.01 L)^2, (0.03 L)^2
};
template <typename T>
inline SsimConsts<T> ssim_consts(T data_range) {
    return {(T(0.01) * data_range) * (T(0.01) * data_range), (T(0.03) * data_range) * (T(0.03) * data_range)};
}

// ------------------------------------------------------------------ pair terms
// One pair (x, f) at one map pixel, from the window moments mu_x, mu_f, sx = max(var x, 0), sf = max(var f, 0), sxf = cov(x, f) and
// kf = [var f > 0]: the quantity Q -- cs = v1 / v2, or ssim = m1 v1 / (m2 v2) -- and its adjoint coefficients
//   A = dQ/d mu_f,  B = dQ/d E[f^2],  C = dQ/d E[x f]      so that   dQ/df = G^T*A + 2 f (G^T*B) + x (G^T*C)
struct SsimPair {
    float Q, A, B, C;
};
// `cs` selects the quantity at run time, as ssimx_stats_kernel needs it: m1 .. v2 stand ahead of ONE branch, and the compiler contracts
// the two arms' multiply-adds as golden F24 pins them.  (As a template flag, two instantiations chosen between by the caller, v1 and v2
// are computed in each arm; the ssim arm then vectorises differently and the gradient's last bits move.)  ssim_stats_kernel of loss.hip
// keeps a copy of the ssim arm: see there.
__device__ __forceinline__ SsimPair ssim_pair_terms(bool cs, float mux, float muf, float sx, float sf, float sxf, float kf, float C1, float C2) {
    const float m1 = 2.f * mux * muf + C1, m2 = mux * mux + muf * muf + C1;
    const float v1 = 2.f * sxf + C2, v2 = sx + sf + C2;
    SsimPair p;
    if (cs) {
        p.Q = v1 / v2;
        p.B = -(p.Q / v2) * kf;
        p.C = 2.f / v2;
        p.A = -mux * p.C - 2.f * muf * p.B;
    } else {
        const float inv = 1.f / (m2 * v2);
        p.Q = m1 * v1 * inv;
        p.B = -(p.Q / v2) * kf;
        p.C = 2.f * m1 * inv;
        p.A = 2.f * mux * v1 * inv - 2.f * muf * p.Q / m2 - 2.f * mux * m1 * inv - 2.f * muf * p.B;
    }
    return p;
}

// ------------------------------------------------------------------ element-wise grids
inline int ew_grid(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------ the 5-level pyramid (MS-SSIM loss: float; MS-SSIM metric: float and double)
constexpr int SSIM_LEVELS = 5;

struct SsimPyramid {
    int h[SSIM_LEVELS], w[SSIM_LEVELS];   // level l + 1 = ceil(level l / 2): 2 x 2 means of the level reflect-padded to even extents
    size_t pixels(int l) const { return (size_t)h[l] * w[l]; }
};
inline SsimPyramid ssim_pyramid(int h, int w) {
    SsimPyramid p;
    p.h[0] = h;
    p.w[0] = w;
    for (int l = 1; l < SSIM_LEVELS; ++l) {
        p.h[l] = (p.h[l - 1] + 1) / 2;
        p.w[l] = (p.w[l - 1] + 1) / 2;
    }
    return p;
}

// dst[y][x] = mean of the 2x2 cell of the source reflect-padded to even size (core/loss.py:146-153, core/metric.py:389-395); h, w >= 2.
// The arithmetic runs in the destination's type TD.
template <typename TD, typename TS = TD>
__global__ void avg_pool_pad_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int n, int h, int w) {
    const int ho = (h + 1) / 2, wo = (w + 1) / 2;
    const long long total = (long long)n * ho * wo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = i % wo, y = (i / wo) % ho, b = i / ((long long)wo * ho);
        const TS* p = src + (long long)b * h * w;
        const int y0 = 2 * y, y1 = (2 * y + 1 < h) ? 2 * y + 1 : h - 2, x0 = 2 * x, x1 = (2 * x + 1 < w) ? 2 * x + 1 : w - 2;
        dst[i] = TD(0.25) * (((TD)p[(long long)y0 * w + x0] + (TD)p[(long long)y0 * w + x1]) +
                             ((TD)p[(long long)y1 * w + x0] + (TD)p[(long long)y1 * w + x1]));
    }
}

// one pyramid step of up to three images [n][h][w] -> [n][ceil(h / 2)][ceil(w / 2)], one launch per image (a null source is skipped),
// then the launch check
template <typename TD, typename TS>
inline int avg_pool_pad3(const TS* const* src, TD* const* dst, int n, int h, int w, hipStream_t st, const char* what) {
    const int grid = ew_grid((long long)n * ((h + 1) / 2) * ((w + 1) / 2));
    for (int q = 0; q < 3; ++q)
        if (src[q] != nullptr) hipLaunchKernelGGL((avg_pool_pad_kernel<TD, TS>), dim3(grid), dim3(256), 0, st, src[q], dst[q], n, h, w);
    return check_launch(what);
}

}  // namespace mmif
