// Mixed depth-wise convolution (MixConvBlock.dwconvs, reference core/block.py:249-273, and lone 5x5 / 7x7 depth-wise ConvLayers): a tensor of
// nseg * c channels, fp32 NCHW; segment i = channels [i c, (i + 1) c) has kernel k_i = k0 + 2 i (odd, <= 7), stride 1, padding k_i / 2,
// reflect | zero.  One launch serves every segment and writes straight into the concatenated tensor; the weights are one packed buffer
// (segment i at float offset c sum_{j<i} k_j^2, layout [c][k_i][k_i]).  include/mmif.h is the contract.
//
//   tile      one block pass = one MD_TH x MD_TW output tile of one plane.  The tile plus its halo of p is staged into LDS once, the
//             reflect | zero index resolved on the load (clamped for the overhang of ragged last tiles): no address leaves the plane.
//   dispatch  k is uniform over a plane, hence over a block pass, and a template parameter of the body: taps unroll and the <= 49 weights
//             of the channel are read at uniform addresses (scalar registers).
//   thread    row r = tid / 16, strip of MD_STRIP = 4 neighbouring outputs; for every tap row the k + 3 window values are read from LDS
//             once (16-byte reads) and slide through the four outputs in registers.
//   LDS pitch MD_PITCH = 128 floats: a wave reads rows r .. r + 3, and the 16-lane groups of a 16-byte LDS read pair lanes 0-3 / 12-15 of
//             one row with lanes 4-11 of the next; with a pitch that is a multiple of 64 dwords those three pieces tile the 64 banks exactly
//             (any pitch in 70 .. 127 makes them overlap).  22 rows x 128 floats = 11 KiB per block.
//   dgrad     the exact adjoint: g is staged with zeros outside the plane; the in-plane image of a pixel is the same sliding window with the
//             taps flipped, the mirror images (pixels within p of an edge, reflect only) are gathered from the same LDS tile.
//   wgrad     stage 1: k^2 + 1 register accumulators per thread over its strip, wave butterfly, the 4 waves added in order, one partial
//             per (sample, tile, channel) in the workspace; stage 2: one block per channel adds the n * tiles partials in a fixed order.
//             No atomics; the grids and every constant depend on the shape only.
#include "common.hpp"

namespace mmif {

constexpr int MD_TH = 16, MD_TW = 64, MD_STRIP = 4;
constexpr int MD_KMAX = 7;
constexpr int MD_PITCH = 128;
constexpr int MD_ROWS = MD_TH + MD_KMAX - 1;
constexpr int MD_SLOTS = MD_KMAX * MD_KMAX + 1;   // workspace floats per (sample, tile, channel): taps at 0 .. k^2 - 1, the bias sum at MD_SLOTS - 1
constexpr int MD_MAX_BLOCKS = 4096;               // forward / dgrad / wgrad stage 1 walk the (plane, tile) list with at most this many blocks

struct MD {
    int n, c, nseg, k0, h, wd, reflect;
    int tiles_x, tiles_y;
};

__host__ __device__ inline int md_woff(int c, int k0, int seg) {
    int o = 0;
    for (int j = 0; j < seg; ++j) o += (k0 + 2 * j) * (k0 + 2 * j);
    return o * c;
}

// tile[ly][lx] = plane[y0 + ly - P][x0 + lx - P] under reflect (index folded, then clamped: the clamp only acts on tile overhang) or zero padding
template <int K>
__device__ inline void md_stage(float* __restrict__ tile, const float* __restrict__ pl, int h, int wd, int y0, int x0, int reflect) {
    constexpr int P = K / 2, W = MD_TW + 2 * P, R = MD_TH + 2 * P;
    for (int e = threadIdx.x; e < R * W; e += 256) {
        const int ly = e / W, lx = e - ly * W;
        int gy = y0 + ly - P, gx = x0 + lx - P;
        float v = 0.f;
        if (reflect) {
            gy = min(max(reflect_idx(gy, h), 0), h - 1);
            gx = min(max(reflect_idx(gx, wd), 0), wd - 1);
            v = pl[(long long)gy * wd + gx];
        } else if (gy >= 0 && gy < h && gx >= 0 && gx < wd) {
            v = pl[(long long)gy * wd + gx];
        }
        tile[ly * MD_PITCH + lx] = v;
    }
}

// the k + 3 window values of tap row `row` for the strip at column 4 s (16-byte aligned: MD_PITCH and 4 s are multiples of 4)
template <int K>
__device__ inline void md_window(const float* __restrict__ tile, int row, int s, float (&win)[12]) {
    const float4* q = reinterpret_cast<const float4*>(tile + row * MD_PITCH + MD_STRIP * s);
    constexpr int NV = (MD_STRIP + K - 1 + 3) / 4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float4 a = q[i];
        win[4 * i] = a.x; win[4 * i + 1] = a.y; win[4 * i + 2] = a.z; win[4 * i + 3] = a.w;
    }
}

// a value that is the same in every lane, kept in a scalar register
__device__ inline float md_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

__device__ inline void md_store4(float* __restrict__ pl, int h, int wd, int oy, int ox, const float (&v)[4], int vec) {
    if (oy >= h) return;
    float* row = pl + (long long)oy * wd;
    if (vec && ox + 3 < wd) {
        *reinterpret_cast<float4*>(row + ox) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < MD_STRIP; ++j)
            if (ox + j < wd) row[ox + j] = v[j];
    }
}

template <int K>
__device__ inline void md_fwd_tile(float* __restrict__ tile, const float* __restrict__ xp, const float* __restrict__ wc, float b, float* __restrict__ yp,
                                   const MD& q, int y0, int x0, int vec) {
    md_stage<K>(tile, xp, q.h, q.wd, y0, x0, q.reflect);
    __syncthreads();
    float wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = md_uniform(wc[t]);
    const int r = threadIdx.x >> 4, s = threadIdx.x & 15;
    float acc[MD_STRIP] = {b, b, b, b};
#pragma unroll
    for (int u = 0; u < K; ++u) {
        float win[12];
        md_window<K>(tile, r + u, s, win);
#pragma unroll
        for (int v = 0; v < K; ++v)
#pragma unroll
            for (int j = 0; j < MD_STRIP; ++j) acc[j] = fmaf(wr[u * K + v], win[j + v], acc[j]);
    }
    md_store4(yp, q.h, q.wd, y0 + r, x0 + MD_STRIP * s, acc, vec);
}

template <int K>
__device__ inline void md_dgrad_tile(float* __restrict__ tile, const float* __restrict__ gp, const float* __restrict__ wc, float* __restrict__ dxp,
                                     const MD& q, int y0, int x0, int vec) {
    constexpr int P = K / 2;
    md_stage<K>(tile, gp, q.h, q.wd, y0, x0, 0);
    __syncthreads();
    float wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = md_uniform(wc[t]);
    const int r = threadIdx.x >> 4, s = threadIdx.x & 15;
    float acc[MD_STRIP] = {0.f, 0.f, 0.f, 0.f};
    // in-plane image: dx[y][x] += w[u][v] g[y + p - u][x + p - v]; LDS row of g row y + p - u is r + (K - 1 - u)
#pragma unroll
    for (int u = 0; u < K; ++u) {
        float win[12];
        md_window<K>(tile, r + u, s, win);
#pragma unroll
        for (int v = 0; v < K; ++v)
#pragma unroll
            for (int j = 0; j < MD_STRIP; ++j) acc[j] = fmaf(wr[(K - 1 - u) * K + (K - 1 - v)], win[j + v], acc[j]);
    }
    if constexpr (K > 1) {
        const int y = y0 + r;
        if (q.reflect && y < q.h) {
            // the mirror images of (y, x) in the padded domain (logical coordinates, < 0 or >= the extent): image 1 = the reflection about
            // the first row / column, image 2 = about the last; every g they touch lies within p of this pixel's own window, i.e. inside
            // the staged tile
            const bool my1 = y >= 1 && y <= P, my2 = y <= q.h - 2 && y >= q.h - 1 - P;
#pragma unroll 1
            for (int j = 0; j < MD_STRIP; ++j) {
                const int x = x0 + MD_STRIP * s + j;
                if (x >= q.wd) break;
                const bool mx1 = x >= 1 && x <= P, mx2 = x <= q.wd - 2 && x >= q.wd - 1 - P;
                if (!(my1 || my2 || mx1 || mx2)) continue;
                float m = 0.f;
                // rows / columns of g that are both in the plane and in the staged tile
                const int oy_lo = max(0, y0 - P), oy_hi = min(q.h, y0 + MD_TH + P) - 1;
                const int ox_lo = max(0, x0 - P), ox_hi = min(q.wd, x0 + MD_TW + P) - 1;
#pragma unroll 1
                for (int ab = 1; ab < 9; ++ab) {
                    const int ia = ab / 3, ib = ab - 3 * ia;
                    if ((ia == 1 && !my1) || (ia == 2 && !my2) || (ib == 1 && !mx1) || (ib == 2 && !mx2)) continue;
                    const int ya = ia == 0 ? y : (ia == 1 ? -y : 2 * (q.h - 1) - y);
                    const int xb = ib == 0 ? x : (ib == 1 ? -x : 2 * (q.wd - 1) - x);
                    // tap u reads g row ya + P - u: only the taps whose row exists (a mirror image keeps at most P of the K rows)
                    const int u_lo = max(0, ya + P - oy_hi), u_hi = min(K - 1, ya + P - oy_lo);
                    const int v_lo = max(0, xb + P - ox_hi), v_hi = min(K - 1, xb + P - ox_lo);
#pragma unroll 1
                    for (int u = u_lo; u <= u_hi; ++u) {
                        const float* trow = tile + (ya + P - u - y0 + P) * MD_PITCH + (xb + P - x0 + P);
#pragma unroll 1
                        for (int v = v_lo; v <= v_hi; ++v) m = fmaf(wc[u * K + v], trow[-v], m);
                    }
                }
                // (a static index keeps acc in registers)
                if (j == 0) acc[0] += m; else if (j == 1) acc[1] += m; else if (j == 2) acc[2] += m; else acc[3] += m;
            }
        }
    }
    md_store4(dxp, q.h, q.wd, y0 + r, x0 + MD_STRIP * s, acc, vec);
}

// partial[slot] of this (sample, tile, channel): slot u K + v = sum over the tile of g x(shifted), slot MD_SLOTS - 1 = sum g
template <int K>
__device__ inline void md_wgrad_tile(float* __restrict__ tile, float* __restrict__ red, const float* __restrict__ xp, const float* __restrict__ gp,
                                     float* __restrict__ part, const MD& q, int y0, int x0) {
    md_stage<K>(tile, xp, q.h, q.wd, y0, x0, q.reflect);
    __syncthreads();
    const int r = threadIdx.x >> 4, s = threadIdx.x & 15;
    const int oy = y0 + r, ox = x0 + MD_STRIP * s;
    float g[MD_STRIP];
#pragma unroll
    for (int j = 0; j < MD_STRIP; ++j) g[j] = (oy < q.h && ox + j < q.wd) ? gp[(long long)oy * q.wd + ox + j] : 0.f;
    float acc[K * K + 1];
    acc[K * K] = ((g[0] + g[1]) + g[2]) + g[3];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        float win[12];
        md_window<K>(tile, r + u, s, win);
#pragma unroll
        for (int v = 0; v < K; ++v) {
            float a = g[0] * win[v];
#pragma unroll
            for (int j = 1; j < MD_STRIP; ++j) a = fmaf(g[j], win[j + v], a);
            acc[u * K + v] = a;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < K * K + 1; ++t) {
        float a = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) red[wave * MD_SLOTS + t] = a;
    }
    __syncthreads();
    if (threadIdx.x < K * K + 1) {
        const int t = threadIdx.x;
        const float a = ((red[t] + red[MD_SLOTS + t]) + red[2 * MD_SLOTS + t]) + red[3 * MD_SLOTS + t];
        part[t == K * K ? MD_SLOTS - 1 : t] = a;
    }
}

enum { MD_FWD = 0, MD_DGRAD = 1, MD_WGRAD = 2 };

// a = x (fwd, wgrad) | gy (dgrad); b = gy (wgrad); out = y | dx | the workspace
template <int MODE>
__global__ __launch_bounds__(256) void mixdw_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ out, MD q, long long total, int vec) {
    __shared__ __attribute__((aligned(16))) float tile[MD_ROWS * MD_PITCH];
    __shared__ float red[4 * MD_SLOTS];
    const int C = q.nseg * q.c, tpp = q.tiles_x * q.tiles_y;
    const long long hw = (long long)q.h * q.wd;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const long long plane = t / tpp;
        const int tl = (int)(t - plane * tpp);
        const int ch = (int)(plane % C), seg = ch / q.c, k = q.k0 + 2 * seg;
        const int y0 = (tl / q.tiles_x) * MD_TH, x0 = (tl % q.tiles_x) * MD_TW;
        const float* wc = w != nullptr ? w + md_woff(q.c, q.k0, seg) + (ch - seg * q.c) * k * k : nullptr;
        const float* ap = a + plane * hw;
        __syncthreads();   // the previous pass has finished with the tile
        if constexpr (MODE == MD_FWD) {
            const float bv = bias != nullptr ? bias[ch] : 0.f;
            float* yp = out + plane * hw;
            switch (k) {
                case 1: md_fwd_tile<1>(tile, ap, wc, bv, yp, q, y0, x0, vec); break;
                case 3: md_fwd_tile<3>(tile, ap, wc, bv, yp, q, y0, x0, vec); break;
                case 5: md_fwd_tile<5>(tile, ap, wc, bv, yp, q, y0, x0, vec); break;
                default: md_fwd_tile<7>(tile, ap, wc, bv, yp, q, y0, x0, vec); break;
            }
        } else if constexpr (MODE == MD_DGRAD) {
            float* dp = out + plane * hw;
            switch (k) {
                case 1: md_dgrad_tile<1>(tile, ap, wc, dp, q, y0, x0, vec); break;
                case 3: md_dgrad_tile<3>(tile, ap, wc, dp, q, y0, x0, vec); break;
                case 5: md_dgrad_tile<5>(tile, ap, wc, dp, q, y0, x0, vec); break;
                default: md_dgrad_tile<7>(tile, ap, wc, dp, q, y0, x0, vec); break;
            }
        } else {
            const float* gp = b + plane * hw;
            // workspace [sample][tile][channel][MD_SLOTS]
            float* part = out + (((plane / C) * tpp + tl) * C + ch) * MD_SLOTS;
            switch (k) {
                case 1: md_wgrad_tile<1>(tile, red, ap, gp, part, q, y0, x0); break;
                case 3: md_wgrad_tile<3>(tile, red, ap, gp, part, q, y0, x0); break;
                case 5: md_wgrad_tile<5>(tile, red, ap, gp, part, q, y0, x0); break;
                default: md_wgrad_tile<7>(tile, red, ap, gp, part, q, y0, x0); break;
            }
        }
    }
}

// one block per channel: wave q adds entries q, q + 4, ... of its slot (lane) in order, then the four waves are added in order
__global__ __launch_bounds__(256) void mixdw_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, MD q,
                                                          long long entries) {
    __shared__ float red[4 * 64];
    const int C = q.nseg * q.c, ch = blockIdx.x, seg = ch / q.c, k = q.k0 + 2 * seg, kk = k * k;
    const int slot = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = slot < kk || slot == MD_SLOTS - 1;
    float s = 0.f;
    if (live)
        for (long long e = wave; e < entries; e += 4) s += ws[(e * C + ch) * MD_SLOTS + slot];
    red[wave * 64 + slot] = s;
    __syncthreads();
    if (wave == 0 && live) {
        const float t = ((red[slot] + red[64 + slot]) + red[128 + slot]) + red[192 + slot];
        if (slot < kk) dw[md_woff(q.c, q.k0, seg) + (ch - seg * q.c) * kk + slot] = t;
        else if (db != nullptr) db[ch] = t;
    }
}

static int md_check(const char* who, int n, int c, int nseg, int k0, int h, int wd, int reflect, MD* q) {
    MMIF_REQUIRE(n > 0 && c > 0 && h > 0 && wd > 0, "%s: bad arguments (n %d, c %d, h %d, w %d)", who, n, c, h, wd);
    MMIF_REQUIRE(k0 >= 1 && (k0 & 1) == 1, "%s: k0 must be odd and >= 1 (got %d)", who, k0);
    MMIF_REQUIRE(nseg >= 1 && nseg <= 4, "%s: nseg must be 1..4 (got %d)", who, nseg);
    const int kmax = k0 + 2 * (nseg - 1);
    MMIF_REQUIRE(kmax <= MD_KMAX, "%s: largest kernel k0 + 2 (nseg - 1) must be <= 7 (got %d)", who, kmax);
    MMIF_REQUIRE(!reflect || (h >= kmax / 2 + 1 && wd >= kmax / 2 + 1), "%s: reflect padding needs h,w >= %d (got %d x %d)", who, kmax / 2 + 1, h, wd);
    const long long tiles = (long long)cdiv(h, MD_TH) * cdiv(wd, MD_TW);
    MMIF_REQUIRE((long long)n * c * nseg * tiles < (1ll << 31) / MD_SLOTS && (long long)c * nseg <= 65535,
                 "%s: too many (plane, tile) pairs or channels (n %d, channels %lld, tiles %lld)", who, n, (long long)c * nseg, tiles);
    q->n = n; q->c = c; q->nseg = nseg; q->k0 = k0; q->h = h; q->wd = wd; q->reflect = reflect ? 1 : 0;
    q->tiles_x = cdiv(wd, MD_TW); q->tiles_y = cdiv(h, MD_TH);
    return MMIF_OK;
}

static inline long long md_total(const MD& q) { return (long long)q.n * q.nseg * q.c * q.tiles_x * q.tiles_y; }
static inline int md_grid(const MD& q) { return (int)(md_total(q) < MD_MAX_BLOCKS ? md_total(q) : MD_MAX_BLOCKS); }
static inline int md_vec(const MD& q, const void* p) { return (q.wd % 4 == 0 && ((uintptr_t)p & 15) == 0) ? 1 : 0; }

}  // namespace mmif

using namespace mmif;

extern "C" int mmif_mixdw_fwd(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c, int32_t nseg, int32_t k0, int32_t h,
                              int32_t wd, int32_t reflect, void* stream) {
    MD q;
    if (int rc = md_check("mixdw_fwd", n, c, nseg, k0, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "mixdw_fwd: null pointer");
    hipLaunchKernelGGL(mixdw_kernel<MD_FWD>, dim3(md_grid(q)), dim3(256), 0, (hipStream_t)stream, x, (const float*)nullptr, w, bias, y, q, md_total(q),
                       md_vec(q, y));
    return check_launch("mixdw_fwd");
}

extern "C" int mmif_mixdw_dgrad(const float* gy, const float* w, float* dx, int32_t n, int32_t c, int32_t nseg, int32_t k0, int32_t h, int32_t wd,
                                int32_t reflect, void* stream) {
    MD q;
    if (int rc = md_check("mixdw_dgrad", n, c, nseg, k0, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(gy != nullptr && w != nullptr && dx != nullptr, "mixdw_dgrad: null pointer");
    hipLaunchKernelGGL(mixdw_kernel<MD_DGRAD>, dim3(md_grid(q)), dim3(256), 0, (hipStream_t)stream, gy, (const float*)nullptr, w, (const float*)nullptr, dx,
                       q, md_total(q), md_vec(q, dx));
    return check_launch("mixdw_dgrad");
}

extern "C" size_t mmif_mixdw_wgrad_workspace(int32_t n, int32_t c, int32_t nseg, int32_t k0, int32_t h, int32_t wd) {
    MD q;
    if (md_check("mixdw_wgrad_workspace", n, c, nseg, k0, h, wd, 0, &q)) return 0;
    return (size_t)md_total(q) * MD_SLOTS * sizeof(float);
}

extern "C" int mmif_mixdw_wgrad(const float* x, const float* gy, float* dw, float* db, int32_t n, int32_t c, int32_t nseg, int32_t k0, int32_t h,
                                int32_t wd, int32_t reflect, void* workspace, size_t workspace_bytes, void* stream) {
    MD q;
    if (int rc = md_check("mixdw_wgrad", n, c, nseg, k0, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(x != nullptr && gy != nullptr && dw != nullptr && workspace != nullptr, "mixdw_wgrad: null pointer");
    const size_t need = (size_t)md_total(q) * MD_SLOTS * sizeof(float);
    if (workspace_bytes < need) {
        set_error("mixdw_wgrad: workspace of %zu bytes, needs %zu", workspace_bytes, need);
        return MMIF_EWORKSPACE;
    }
    hipLaunchKernelGGL(mixdw_kernel<MD_WGRAD>, dim3(md_grid(q)), dim3(256), 0, (hipStream_t)stream, x, gy, (const float*)nullptr, (const float*)nullptr,
                       (float*)workspace, q, md_total(q), 0);
    if (int rc = check_launch("mixdw_wgrad")) return rc;
    hipLaunchKernelGGL(mixdw_wgrad_reduce, dim3(q.nseg * q.c), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, db, q,
                       (long long)q.n * q.tiles_x * q.tiles_y);
    return check_launch("mixdw_wgrad_reduce");
}
