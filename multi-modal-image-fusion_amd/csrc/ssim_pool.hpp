// The pyramid step shared by the MS-SSIM loss (loss_modes.hip, float) and the MS-SSIM metric (metric_ssim.hip, double).
#pragma once
#include "common.hpp"

namespace mmif {

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

}  // namespace mmif
