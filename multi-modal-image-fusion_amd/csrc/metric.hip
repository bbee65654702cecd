// Fusion-quality metrics of eval.py (reference core/metric.py): per-SAMPLE raw terms, finished on the host side (core/metric.py of
// this package) into the reference's per-image or pooled values.
//   moments  :25-100   means, centred Gram matrix, AG and SF sums of k = 1..3 images (MSE, SD, CC, SCD follow)
//   hist     :103-166  256-bin histograms of x and y and the 256x256 joint histogram (u32 counts, integer atomics: exact in any order)
//   entropy  :119-190  EN(x), EN(y), joint entropy, CE(x||y) from the counts, fp64
//   qabf     :192-287  the five Qabf / Nabf / Labf sums of a triple, Sobel + atan2 + sigmoids of all three images from one LDS tile
//   vif      :406-491  per scale: sum N1, D1, N2, D2 and the g1 < g2 selected num / den, both pairs at the same pixel
// (MS-SSIM runs on the loss's SSIM kernels and pyramid: mmif_metric_msssim in loss_modes.hip.)
// Every floating-point sum is a per-block fp64 partial followed by a fixed-order second stage (rows_sum_d_kernel), and the block
// grid over one sample depends on h and w only: a sample's result is bit-identical from run to run and whatever batch it is in.
// The per-pixel maths is fp64 wherever the reference's branches compare against small thresholds (VIF's eps = 1e-10 on variances,
// Qabf's sign of a Sobel response through atan2): fp64 products of the fp32 inputs are exact, so those decisions match the
// reference's fp64 run.
#include <math.h>

#include "common.hpp"

namespace mmif {

__device__ inline double block_sum_d(double v, double* smem /* >= 16 doubles */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r += smem[i];
    }
    return r;
}

// out[r] = sum_{i < nblk} partial[r * nblk + i], one block per row, fixed order
__global__ __launch_bounds__(256) void rows_sum_d_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partial[(long long)blockIdx.x * nblk + i];
    const double t = block_sum_d(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

struct Imgs3 {
    const float* p[3];
};

static int sample_blocks(long long hw) {   // grid over one sample: a function of the image size only
    long long b = (hw + 2047) / 2048;
    return (int)(b < 1 ? 1 : (b > 128 ? 128 : b));
}

// ------------------------------------------------------------------ moments
// pass 1: partial[s][i][blk] = sum x_i
__global__ __launch_bounds__(256) void moments_sum_kernel(Imgs3 im, int k, long long hw, double* __restrict__ partial) {
    __shared__ double red[16];
    const int s = blockIdx.y, nblk = gridDim.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long long)nblk * 256)
        for (int j = 0; j < k; ++j) acc[j] += (double)im.p[j][(long long)s * hw + i];
    for (int j = 0; j < k; ++j) {
        const double t = block_sum_d(acc[j], red);
        if (threadIdx.x == 0) partial[((long long)s * k + j) * nblk + blockIdx.x] = t;
    }
}

// pass 2: per image pair j <= l the centred product sum, per image the AG sum ((h-1)(w-1) terms), sum dy^2 ((h-1) w), sum dx^2 (h (w-1))
// quantity order: [gram pairs k(k+1)/2 (j-major)] [ag k] [sfr k] [sfc k]
__global__ __launch_bounds__(256) void moments_kernel(Imgs3 im, int k, int h, int w, const double* __restrict__ sums,
                                                      double* __restrict__ partial) {
    __shared__ double red[16];
    const int s = blockIdx.y, nblk = gridDim.x;
    const long long hw = (long long)h * w;
    const double inv = 1.0 / (double)hw;
    double mu[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < k; ++j) mu[j] = sums[s * k + j] * inv;
    double gram[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ag[3] = {0.0, 0.0, 0.0}, sfr[3] = {0.0, 0.0, 0.0}, sfc[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long long)nblk * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        double c[3];
        for (int j = 0; j < k; ++j) {
            const float* p = im.p[j] + (long long)s * hw;
            const double v = (double)p[i];
            c[j] = v - mu[j];
            const double dx = x + 1 < w ? (double)p[i + 1] - v : 0.0;
            const double dy = y + 1 < h ? (double)p[i + w] - v : 0.0;
            if (x + 1 < w && y + 1 < h) ag[j] += sqrt((dx * dx + dy * dy) * 0.5);
            sfr[j] += dy * dy;
            sfc[j] += dx * dx;
        }
        int q = 0;
        for (int j = 0; j < k; ++j)
            for (int l = j; l < k; ++l) gram[q++] += c[j] * c[l];
    }
    const int ng = k * (k + 1) / 2, nq = ng + 3 * k;
    double* dst = partial + (long long)s * nq * nblk + blockIdx.x;
    for (int q = 0; q < ng; ++q) {
        const double t = block_sum_d(gram[q], red);
        if (threadIdx.x == 0) dst[(long long)q * nblk] = t;
    }
    for (int j = 0; j < k; ++j) {
        const double t0 = block_sum_d(ag[j], red);
        if (threadIdx.x == 0) dst[(long long)(ng + j) * nblk] = t0;
        const double t1 = block_sum_d(sfr[j], red);
        if (threadIdx.x == 0) dst[(long long)(ng + k + j) * nblk] = t1;
        const double t2 = block_sum_d(sfc[j], red);
        if (threadIdx.x == 0) dst[(long long)(ng + 2 * k + j) * nblk] = t2;
    }
}

// out[s] = [means k][gram k x k][ag k][sfr k][sfc k]
__global__ void moments_finish_kernel(const double* __restrict__ sums, const double* __restrict__ q, int n, int k, double inv,
                                      double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int ng = k * (k + 1) / 2, nq = ng + 3 * k, no = k + k * k + 3 * k;
    double* o = out + (long long)s * no;
    const double* qs = q + (long long)s * nq;
    for (int j = 0; j < k; ++j) o[j] = sums[s * k + j] * inv;
    int g = 0;
    for (int j = 0; j < k; ++j)
        for (int l = j; l < k; ++l) {
            o[k + j * k + l] = qs[g];
            o[k + l * k + j] = qs[g];
            ++g;
        }
    for (int j = 0; j < 3 * k; ++j) o[k + k * k + j] = qs[ng + j];
}

// ------------------------------------------------------------------ histograms
// torch.histc(x, 256, 0, 256) / np.histogram2d(.., ((0, 256), (0, 256))): bin floor(x) on [0, 256), 256 -> 255, else (and NaN) dropped
__device__ inline int hist_bin(float v) {
    if (!(v >= 0.f && v <= 256.f)) return -1;
    const int b = (int)v;
    return b > 255 ? 255 : b;
}

constexpr int HSLAB = 64;   // x-bin rows of the joint histogram per block: 64 x 256 u32 = 64 KiB of LDS

// grid (chunks, 256 / HSLAB, n): the block of slab z sweeps its pixel chunk and counts the joint pairs whose x-bin lies in its slab
// (and, slab 0 only, both marginals) in LDS, then adds its non-zero bins to the global counts
__global__ __launch_bounds__(256) void hist_kernel(const float* __restrict__ x, const float* __restrict__ y, long long hw, int chunk,
                                                   uint32_t* __restrict__ hx, uint32_t* __restrict__ hy, uint32_t* __restrict__ hxy) {
    __shared__ uint32_t joint[HSLAB * 256];
    __shared__ uint32_t mx[256], my[256];
    const int s = blockIdx.z, slab = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < HSLAB * 256; i += 256) joint[i] = 0u;
    mx[tid] = 0u;
    my[tid] = 0u;
    __syncthreads();
    const long long b0 = (long long)blockIdx.x * chunk, b1 = b0 + chunk < hw ? b0 + chunk : hw;
    const float* xs = x + (long long)s * hw;
    const float* ys = y + (long long)s * hw;
    const int lo = slab * HSLAB;
    for (long long i = b0 + tid; i < b1; i += 256) {
        const int bx = hist_bin(xs[i]), by = hist_bin(ys[i]);
        if (slab == 0) {
            if (bx >= 0) atomicAdd(&mx[bx], 1u);
            if (by >= 0) atomicAdd(&my[by], 1u);
        }
        if (bx >= lo && bx < lo + HSLAB && by >= 0) atomicAdd(&joint[(bx - lo) * 256 + by], 1u);
    }
    __syncthreads();
    uint32_t* gj = hxy + (long long)s * 65536 + (long long)lo * 256;
    for (int i = tid; i < HSLAB * 256; i += 256)
        if (joint[i] != 0u) atomicAdd(&gj[i], joint[i]);
    if (slab == 0) {
        if (mx[tid] != 0u) atomicAdd(&hx[s * 256 + tid], mx[tid]);
        if (my[tid] != 0u) atomicAdd(&hy[s * 256 + tid], my[tid]);
    }
}

// ------------------------------------------------------------------ entropies, one block of 256 per sample
// out[s] = EN(x), EN(y), joint entropy, CE(x||y); p = count / numel (numel includes the dropped values, as the reference)
__global__ __launch_bounds__(256) void entropy_kernel(const uint32_t* __restrict__ hx, const uint32_t* __restrict__ hy,
                                                      const uint32_t* __restrict__ hxy, double numel, double* __restrict__ out) {
    __shared__ double red[16];
    const int s = blockIdx.x, t = threadIdx.x;
    const double p1 = (double)hx[s * 256 + t] / numel, p2 = (double)hy[s * 256 + t] / numel;
    const double e1 = p1 != 0.0 ? -p1 * log2(p1) : 0.0;
    const double e2 = p2 != 0.0 ? -p2 * log2(p2) : 0.0;
    const double ce = p1 * p2 != 0.0 ? p1 * log2(p1 / p2) : 0.0;
    double ej = 0.0;
    const uint32_t* row = hxy + (long long)s * 65536 + (long long)t * 256;
    for (int j = 0; j < 256; ++j) {
        const double p = (double)row[j] / numel;
        if (p != 0.0) ej -= p * log2(p);
    }
    const double v[4] = {e1, e2, ej, ce};
    for (int q = 0; q < 4; ++q) {
        const double r = block_sum_d(v[q], red);
        if (t == 0) out[s * 4 + q] = r;
    }
}

// ------------------------------------------------------------------ Qabf family
constexpr int QT = 16;   // output tile edge; the LDS tile carries a 1-px reflect halo of all three images

__device__ inline int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ inline void sobel(const float (*t)[QT + 3], int py, int px, double& g, double& a) {
    // cross-correlation with [[-1,0,1],[-2,0,2],[-1,0,1]] and its transpose (core/metric.py:234-248)
    const double gx = ((double)t[py][px + 2] - t[py][px]) + 2.0 * ((double)t[py + 1][px + 2] - t[py + 1][px]) +
                      ((double)t[py + 2][px + 2] - t[py + 2][px]);
    const double gy = ((double)t[py + 2][px] - t[py][px]) + 2.0 * ((double)t[py + 2][px + 1] - t[py][px + 1]) +
                      ((double)t[py + 2][px + 2] - t[py][px + 2]);
    g = sqrt(gx * gx + gy * gy);
    a = atan2(gy, gx);
}

__device__ inline double qxy(double g1, double a1, double g2, double a2) {
    const double PI = 3.141592653589793;
    double G = fmin(g1, g2) / fmax(g1, g2);
    if (G != G) G = 0.0;   // 0 / 0
    const double A = fabs(fabs(a1 - a2) - PI / 2) * 2 / PI;
    const double Qg = 0.9994 / (1.0 + exp(-15.0 * (G - 0.5)));
    const double Qa = 0.9879 / (1.0 + exp(-22.0 * (A - 0.8)));
    return Qg * Qa;
}

// partial[s][q][blk]: q0 sum(Qaf wa + Qbf wb), q1 sum(wa + wb), q2 sum AM((1-Qaf) wa + (1-Qbf) wb), q3 the same under RR,
// q4 sum AM (2 - Qaf - Qbf)(wa + wb)
__global__ __launch_bounds__(256) void qabf_kernel(Imgs3 im, int h, int w, double L, int tiles_x, double* __restrict__ partial) {
    __shared__ float t[3][QT + 2][QT + 3];
    __shared__ double red[16];
    const int s = blockIdx.y, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = (blockIdx.x % tiles_x) * QT, y0 = (blockIdx.x / tiles_x) * QT;
    const long long base = (long long)s * h * w;
    for (int e = tid; e < (QT + 2) * (QT + 2); e += 256) {
        const int py = e / (QT + 2), px = e % (QT + 2);
        int yy = y0 + py - 1, xx = x0 + px - 1;
        yy = yy >= h + 1 ? h - 1 : reflect1(yy, h);   // rows/cols past the image's end + 1 feed only outputs that are not counted
        xx = xx >= w + 1 ? w - 1 : reflect1(xx, w);
        const long long i = base + (long long)yy * w + xx;
        for (int j = 0; j < 3; ++j) t[j][py][px] = im.p[j][i];
    }
    __syncthreads();
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (y0 + ty < h && x0 + tx < w) {
        double ga, aa, gb, ab, gf, af;
        sobel(t[0], ty, tx, ga, aa);
        sobel(t[1], ty, tx, gb, ab);
        sobel(t[2], ty, tx, gf, af);
        const double qaf = qxy(ga, aa, gf, af), qbf = qxy(gb, ab, gf, af);
        const double wa = pow(ga, L), wb = pow(gb, L);
        const double gm = fmax(ga, gb);
        const double loss = (1.0 - qaf) * wa + (1.0 - qbf) * wb;
        v[0] = qaf * wa + qbf * wb;
        v[1] = wa + wb;
        if (gf > gm) {
            v[2] = loss;
            v[4] = (2.0 - qaf - qbf) * (wa + wb);
        }
        if (gf <= gm) v[3] = loss;
    }
    const int nblk = gridDim.x;
    for (int q = 0; q < 5; ++q) {
        const double r = block_sum_d(v[q], red);
        if (tid == 0) partial[((long long)s * 5 + q) * nblk + blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------ VIF
// window of scale s: K = 2^(5-s) + 1 taps t (fp32, the reference's create_window), 2-D weight = fp32 product t[u] * t[v]
struct VifWin {
    float w[17 * 17];
};
constexpr int VT = 16;

// dst = (valid correlation of src with the window)[::2, ::2] for the three images (fp64 levels)
template <typename T, int K>
__global__ __launch_bounds__(256) void vif_down_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ f, int h,
                                                       int w, VifWin win, double* __restrict__ da, double* __restrict__ db,
                                                       double* __restrict__ df, int ho, int wo) {
    const int s = blockIdx.y;
    const long long tot = (long long)ho * wo;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long long)gridDim.x * 256) {
        const int oy = (int)(i / wo), ox = (int)(i % wo);
        const long long o = (long long)s * h * w + (long long)(2 * oy) * w + 2 * ox;
        double r[3] = {0.0, 0.0, 0.0};
        for (int u = 0; u < K; ++u)
            for (int v = 0; v < K; ++v) {
                const double wt = (double)win.w[u * K + v];
                const long long j = o + (long long)u * w + v;
                r[0] += wt * (double)a[j];
                r[1] += wt * (double)b[j];
                r[2] += wt * (double)f[j];
            }
        const long long d = (long long)s * tot + i;
        da[d] = r[0];
        db[d] = r[1];
        df[d] = r[2];
    }
}

// the branch updates of core/metric.py:478-494 in the reference's order; -> N, D, g of one pair at one pixel
__device__ inline void vif_pair(double mux, double muf, double exx, double eff, double exf, double& N, double& D, double& g) {
    const double eps = 1e-10, sn = 0.005 * 255 * 255;
    double s1 = exx - mux * mux, s2 = eff - muf * muf;
    const double s12 = exf - mux * muf;
    if (s1 < 0) s1 = 0.0;
    if (s2 < 0) s2 = 0.0;
    g = s12 / (s1 + eps);
    double sv = s2 - g * s12;
    if (s1 < eps) {
        g = 0.0;
        sv = s2;
        s1 = 0.0;
    }
    if (s2 < eps) {
        g = 0.0;
        sv = 0.0;
    }
    if (g < 0) {
        sv = s2;
        g = 0.0;
    }
    if (sv < eps) sv = eps;
    N = log2(1.0 + g * g * s1 / (sv + sn));
    D = log2(1.0 + s1 / sn);
}

// partial[s][q][blk]: q0 sum N1, q1 sum D1, q2 sum N2, q3 sum D2, q4 sum (g1 < g2 ? N1 : N2), q5 sum (g1 < g2 ? D1 : D2)
template <typename T, int K>
__global__ __launch_bounds__(256) void vif_stats_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ f, int h,
                                                        int w, VifWin win, int tiles_x, double* __restrict__ partial) {
    constexpr int LT = VT + K - 1;
    __shared__ double t[3][LT][LT + 1];
    __shared__ double red[16];
    const int s = blockIdx.y, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = (blockIdx.x % tiles_x) * VT, y0 = (blockIdx.x / tiles_x) * VT;
    const long long base = (long long)s * h * w;
    for (int e = tid; e < LT * LT; e += 256) {
        const int py = e / LT, px = e % LT;
        const int yy = y0 + py, xx = x0 + px;
        const bool ok = yy < h && xx < w;
        const long long i = base + (long long)yy * w + xx;
        t[0][py][px] = ok ? (double)a[i] : 0.0;
        t[1][py][px] = ok ? (double)b[i] : 0.0;
        t[2][py][px] = ok ? (double)f[i] : 0.0;
    }
    __syncthreads();
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (y0 + ty < h - K + 1 && x0 + tx < w - K + 1) {
        double m[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int u = 0; u < K; ++u)
#pragma unroll
            for (int vv = 0; vv < K; ++vv) {
                const double wt = (double)win.w[u * K + vv];
                const double pa = t[0][ty + u][tx + vv], pb = t[1][ty + u][tx + vv], pf = t[2][ty + u][tx + vv];
                m[0] += wt * pa;
                m[1] += wt * pb;
                m[2] += wt * pf;
                m[3] += wt * (pa * pa);
                m[4] += wt * (pb * pb);
                m[5] += wt * (pf * pf);
                m[6] += wt * (pa * pf);
                m[7] += wt * (pb * pf);
            }
        double N1, D1, g1, N2, D2, g2;
        vif_pair(m[0], m[2], m[3], m[5], m[6], N1, D1, g1);
        vif_pair(m[1], m[2], m[4], m[5], m[7], N2, D2, g2);
        v[0] = N1;
        v[1] = D1;
        v[2] = N2;
        v[3] = D2;
        v[4] = g1 < g2 ? N1 : N2;
        v[5] = g1 < g2 ? D1 : D2;
    }
    const int nblk = gridDim.x;
    for (int q = 0; q < 6; ++q) {
        const double r = block_sum_d(v[q], red);
        if (tid == 0) partial[((long long)s * 6 + q) * nblk + blockIdx.x] = r;
    }
}

// level sizes of the VIF pyramid; false if an image is below the reference's minimum (41 x 41)
static bool vif_sizes(int h, int w, int hs[4], int ws[4]) {
    hs[0] = h;
    ws[0] = w;
    for (int sc = 1; sc < 4; ++sc) {
        const int k = (1 << (4 - sc)) + 1;
        hs[sc] = (hs[sc - 1] - k + 2) / 2;   // ceil((n - k + 1) / 2)
        ws[sc] = (ws[sc - 1] - k + 2) / 2;
    }
    for (int sc = 0; sc < 4; ++sc) {
        const int k = (1 << (4 - sc)) + 1;
        if (hs[sc] < k || ws[sc] < k) return false;
    }
    return true;
}

static int vif_tiles(int h, int w, int k, int* tx) {
    *tx = cdiv(w - k + 1, VT);
    return *tx * cdiv(h - k + 1, VT);
}

}  // namespace mmif

using namespace mmif;

// ------------------------------------------------------------------ C ABI
extern "C" size_t mmif_metric_moments_workspace(int32_t n, int32_t h, int32_t w, int32_t k) {
    if (n <= 0 || h <= 0 || w <= 0 || k < 1 || k > 3) return 0;
    const size_t nblk = sample_blocks((long long)h * w), nq = k * (k + 1) / 2 + 3 * k;
    return ((size_t)n * k * nblk + (size_t)n * k + (size_t)n * nq * nblk + (size_t)n * nq) * sizeof(double);
}

extern "C" int mmif_metric_moments(const float* const* imgs, int32_t k, int32_t n, int32_t h, int32_t w, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(k >= 1 && k <= 3, "metric_moments: k must be 1, 2 or 3 (got %d)", k);
    MMIF_REQUIRE(imgs && out && workspace, "metric_moments: NULL argument");
    for (int j = 0; j < k; ++j) MMIF_REQUIRE(imgs[j], "metric_moments: NULL image %d", j);
    MMIF_REQUIRE(n > 0 && h >= 2 && w >= 2, "metric_moments: images must be at least 2x2 (got n=%d %dx%d)", n, h, w);
    if (workspace_bytes < mmif_metric_moments_workspace(n, h, w, k)) {
        set_error("metric_moments: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)h * w;
    const int nblk = sample_blocks(hw), nq = k * (k + 1) / 2 + 3 * k;
    Imgs3 im{{imgs[0], k > 1 ? imgs[1] : imgs[0], k > 2 ? imgs[2] : imgs[0]}};
    double* p1 = (double*)workspace;
    double* s1 = p1 + (size_t)n * k * nblk;
    double* p2 = s1 + (size_t)n * k;
    double* s2 = p2 + (size_t)n * nq * nblk;
    hipLaunchKernelGGL(moments_sum_kernel, dim3(nblk, n), dim3(256), 0, st, im, k, hw, p1);
    hipLaunchKernelGGL(rows_sum_d_kernel, dim3(n * k), dim3(256), 0, st, p1, nblk, s1);
    hipLaunchKernelGGL(moments_kernel, dim3(nblk, n), dim3(256), 0, st, im, k, h, w, s1, p2);
    hipLaunchKernelGGL(rows_sum_d_kernel, dim3(n * nq), dim3(256), 0, st, p2, nblk, s2);
    hipLaunchKernelGGL(moments_finish_kernel, dim3(cdiv(n, 64)), dim3(64), 0, st, s1, s2, n, k, 1.0 / (double)hw, out);
    return check_launch("metric_moments");
}

extern "C" int mmif_metric_hist(const float* x, const float* y, int32_t n, int32_t h, int32_t w, uint32_t* hx, uint32_t* hy,
                                uint32_t* hxy, void* stream) {
    MMIF_REQUIRE(x && y && hx && hy && hxy, "metric_hist: NULL argument");
    MMIF_REQUIRE(n > 0 && h > 0 && w > 0, "metric_hist: empty images (n=%d %dx%d)", n, h, w);
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)h * w;
    (void)hipMemsetAsync(hx, 0, (size_t)n * 256 * sizeof(uint32_t), st);
    (void)hipMemsetAsync(hy, 0, (size_t)n * 256 * sizeof(uint32_t), st);
    (void)hipMemsetAsync(hxy, 0, (size_t)n * 65536 * sizeof(uint32_t), st);
    const int chunk = 16384, nch = cdiv(hw, chunk);
    hipLaunchKernelGGL(hist_kernel, dim3(nch, 256 / HSLAB, n), dim3(256), 0, st, x, y, hw, chunk, hx, hy, hxy);
    return check_launch("metric_hist");
}

extern "C" int mmif_metric_entropy(const uint32_t* hx, const uint32_t* hy, const uint32_t* hxy, int32_t n, int64_t numel, double* out,
                                   void* stream) {
    MMIF_REQUIRE(hx && hy && hxy && out, "metric_entropy: NULL argument");
    MMIF_REQUIRE(n > 0 && numel > 0, "metric_entropy: n and numel must be positive (n=%d numel=%lld)", n, (long long)numel);
    hipLaunchKernelGGL(entropy_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, hx, hy, hxy, (double)numel, out);
    return check_launch("metric_entropy");
}

extern "C" size_t mmif_metric_qabf_workspace(int32_t n, int32_t h, int32_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const size_t tiles = (size_t)cdiv(h, QT) * cdiv(w, QT);
    return (size_t)n * 5 * tiles * sizeof(double);
}

extern "C" int mmif_metric_qabf(const float* a, const float* b, const float* f, int32_t n, int32_t h, int32_t w, double L, double* out,
                                void* workspace, size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(a && b && f && out && workspace, "metric_qabf: NULL argument");
    MMIF_REQUIRE(n > 0 && h >= 2 && w >= 2, "metric_qabf: images must be at least 2x2 for the reflect-padded Sobel (got n=%d %dx%d)", n, h, w);
    if (workspace_bytes < mmif_metric_qabf_workspace(n, h, w)) {
        set_error("metric_qabf: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int tx = cdiv(w, QT), nt = tx * cdiv(h, QT);
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(qabf_kernel, dim3(nt, n), dim3(256), 0, st, Imgs3{{a, b, f}}, h, w, L, tx, partial);
    hipLaunchKernelGGL(rows_sum_d_kernel, dim3(n * 5), dim3(256), 0, st, partial, nt, out);
    return check_launch("metric_qabf");
}

extern "C" size_t mmif_metric_vif_workspace(int32_t n, int32_t h, int32_t w) {
    int hs[4], ws[4];
    if (n <= 0 || !vif_sizes(h, w, hs, ws)) return 0;
    size_t d = 0;
    for (int sc = 0; sc < 4; ++sc) {
        int tx;
        if (sc > 0) d += 3 * (size_t)n * hs[sc] * ws[sc];
        d += (size_t)n * 6 * vif_tiles(hs[sc], ws[sc], (1 << (4 - sc)) + 1, &tx);
    }
    return d * sizeof(double);
}

template <typename T, int K>
static void vif_scale(const T* a, const T* b, const T* f, int n, int h, int w, const VifWin& win, double* partial, double* out,
                      hipStream_t st) {
    int tx;
    const int nt = vif_tiles(h, w, K, &tx);
    hipLaunchKernelGGL((vif_stats_kernel<T, K>), dim3(nt, n), dim3(256), 0, st, a, b, f, h, w, win, tx, partial);
    hipLaunchKernelGGL(rows_sum_d_kernel, dim3(n * 6), dim3(256), 0, st, partial, nt, out);
}
template <typename T, int K>
static void vif_down(const T* a, const T* b, const T* f, int n, int h, int w, const VifWin& win, double* da, double* db, double* df,
                     int ho, int wo, hipStream_t st) {
    const int g = cdiv((long long)ho * wo, 256);
    hipLaunchKernelGGL((vif_down_kernel<T, K>), dim3(g > 1024 ? 1024 : g, n), dim3(256), 0, st, a, b, f, h, w, win, da, db, df, ho, wo);
}

extern "C" int mmif_metric_vif(const float* a, const float* b, const float* f, int32_t n, int32_t h, int32_t w, const float* taps,
                               double* out, void* workspace, size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(a && b && f && taps && out && workspace, "metric_vif: NULL argument");
    int hs[4], ws[4];
    MMIF_REQUIRE(n > 0 && vif_sizes(h, w, hs, ws), "metric_vif: images must be at least 41x41 (got n=%d %dx%d)", n, h, w);
    if (workspace_bytes < mmif_metric_vif_workspace(n, h, w)) {
        set_error("metric_vif: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    VifWin win[4];
    int off = 0;
    for (int sc = 0; sc < 4; ++sc) {
        const int k = (1 << (4 - sc)) + 1;
        for (int u = 0; u < k; ++u)
            for (int v = 0; v < k; ++v) win[sc].w[u * k + v] = taps[off + u] * taps[off + v];
        off += k;
    }
    double* d = (double*)workspace;
    double* lv[4][3];
    for (int sc = 1; sc < 4; ++sc)
        for (int j = 0; j < 3; ++j) {
            lv[sc][j] = d;
            d += (size_t)n * hs[sc] * ws[sc];
        }
    double* part[4];
    for (int sc = 0; sc < 4; ++sc) {
        int tx;
        part[sc] = d;
        d += (size_t)n * 6 * vif_tiles(hs[sc], ws[sc], (1 << (4 - sc)) + 1, &tx);
    }
    // out[s][scale][6] is written scale-major per row block: rows_sum writes out + scale * n * 6, re-laid by the caller
    vif_scale<float, 17>(a, b, f, n, h, w, win[0], part[0], out, st);
    vif_down<float, 9>(a, b, f, n, h, w, win[1], lv[1][0], lv[1][1], lv[1][2], hs[1], ws[1], st);
    vif_scale<double, 9>(lv[1][0], lv[1][1], lv[1][2], n, hs[1], ws[1], win[1], part[1], out + 6 * n, st);
    vif_down<double, 5>(lv[1][0], lv[1][1], lv[1][2], n, hs[1], ws[1], win[2], lv[2][0], lv[2][1], lv[2][2], hs[2], ws[2], st);
    vif_scale<double, 5>(lv[2][0], lv[2][1], lv[2][2], n, hs[2], ws[2], win[2], part[2], out + 12 * n, st);
    vif_down<double, 3>(lv[2][0], lv[2][1], lv[2][2], n, hs[2], ws[2], win[3], lv[3][0], lv[3][1], lv[3][2], hs[3], ws[3], st);
    vif_scale<double, 3>(lv[3][0], lv[3][1], lv[3][2], n, hs[3], ws[3], win[3], part[3], out + 18 * n, st);
    return check_launch("metric_vif");
}
