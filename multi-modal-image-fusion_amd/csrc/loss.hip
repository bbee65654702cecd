// Fusion losses on fp32 images [n][h][w]: SSIM (11x11 Gaussian, valid), max/avg pixel L1/L2,
// Sobel-gradient L1/L2 -- each computes the loss value AND its gradient w.r.t. the fused image
// in the same call (reference: core/loss.py:52-110,240-344,361-385; maths in DESIGN.md / SURVEY A.4-A.5).
// All reductions: per-block partial (wave shuffles + LDS) -> fixed-order second stage; no float atomics.
// The SSIM window taps, map extent and constants are those of csrc/ssim_common.hpp, shared with loss_modes.hip and metric_ssim.hip.
#include <math.h>

#include "common.hpp"
#include "ssim_common.hpp"

namespace mmif {

constexpr int LT = 16;            // tile edge
constexpr int WIN = 11;

// ------------------------------------------------------------------ SSIM, pass 1
// per map pixel: S(x1,f) + S(x2,f) (block partial) and the adjoint inputs
//   mA = Ap1 + Ap2, mB = Bp1 + Bp2, mC1 = Cp1, mC2 = Cp2   
// 32 x 32 map pixels per block (round 2; 16 x 16 with one output per thread and a scalar LDS read per tap was LDS-issue bound:
// 142 reads per pixel).  Both passes slide the 11-tap window over registers: a thread of the horizontal pass owns 4 adjacent
// columns of one row for 4 of the 8 quantities (16 floats of two images in, 4 x 4 sums out), a thread of the vertical pass one
// column x 4 rows for all 8 (14 rows in) -- 33 LDS instructions per pixel.  Every sum keeps the tap order k = 0..10 of the
// 16 x 16 version, so map values and gradients are bit-identical to it; only the order of the block partials changed.
constexpr int ST = 32;                // tile edge
constexpr int SIN = ST + WIN - 1;     // 42
constexpr int SPI = 44;               // row pitch of the staged images (floats; rows stay 16-byte aligned)
constexpr int SPH = 36;               // row pitch of the horizontal sums

typedef float lf32x2 __attribute__((ext_vector_type(2)));

__device__ inline void ld16(const float* p, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 q = *reinterpret_cast<const float4*>(p + 4 * i);
        v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
}

__global__ __launch_bounds__(256, 2) void ssim_stats_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                            const float* __restrict__ f, int H, int W, SsimTaps win, float C1,
                                                            float C2, float* __restrict__ maps /* [4][n][Hm][Wm] or null */,
                                                            float* __restrict__ partial, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float in[3][SIN][SPI];
    __shared__ __attribute__((aligned(16))) float hb[8][SIN][SPH];
    __shared__ float red[16];
    const int Hm = H - WIN + 1, Wm = W - WIN + 1;   // ssim_map_extent(., WIN, 0), spelled out: these two kernels' code is pinned
    const int tid = threadIdx.x;
    const int mx0 = (blockIdx.x % tiles_x) * ST, my0 = (blockIdx.x / tiles_x) * ST;
    const int in_ = blockIdx.y;
    const long long ibase = (long long)in_ * H * W;
    for (int e = tid; e < SIN * SPI; e += 256) {
        const int py = e / SPI, px = e % SPI;
        const int y = my0 + py, x = mx0 + px;
        const bool ok = (y < H) && (x < W) && px < SIN;
        const long long i = ibase + (long long)min(y, H - 1) * W + min(x, W - 1);
        const float a = x1[i], b = x2[i], c = f[i];
        in[0][py][px] = ok ? a : 0.f;
        in[1][py][px] = ok ? b : 0.f;
        in[2][py][px] = ok ? c : 0.f;
    }
    __syncthreads();
    // horizontal pass: item = (set, row, column group of 4); set 0 -> {x1, x1^2, x1 f, f}, set 1 -> {x2, x2^2, x2 f, f^2};
    // each set is padded to whole waves (336 -> 384 items)
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
        const int it = tid + 256 * r, set = it / 384, idx = it - set * 384;
        if (idx >= SIN * 8) continue;
        const int py = idx >> 3, cg = idx & 7;
        float xa[16], fc[16];
        ld16(&in[set][py][4 * cg], xa);
        ld16(&in[2][py][4 * cg], fc);
        // the four quantities of a position as two register pairs (a, a^2), (a c, c | c^2), formed once per position; the 11 taps
        // are then 2 v_pk_fma_f32 per (tap, column) instead of 2 multiplies + 4 FMAs (same products, same order per sum)
        lf32x2 pa[14], pc[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) {
            const float a = xa[i], c = fc[i];
            pa[i] = (lf32x2){a, a * a};
            pc[i] = (lf32x2){a * c, set ? c * c : c};
        }
        lf32x2 s01[4], s23[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s01[j] = s23[j] = (lf32x2){0.f, 0.f};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const lf32x2 wk = (lf32x2){win.t[k], win.t[k]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s01[j] = __builtin_elementwise_fma(wk, pa[j + k], s01[j]);
                s23[j] = __builtin_elementwise_fma(wk, pc[j + k], s23[j]);
            }
        }
        const int q0 = set ? 1 : 0, q1 = set ? 4 : 3, q2 = set ? 7 : 6, q3 = set ? 5 : 2;
        *reinterpret_cast<float4*>(&hb[q0][py][4 * cg]) = make_float4(s01[0].x, s01[1].x, s01[2].x, s01[3].x);
        *reinterpret_cast<float4*>(&hb[q1][py][4 * cg]) = make_float4(s01[0].y, s01[1].y, s01[2].y, s01[3].y);
        *reinterpret_cast<float4*>(&hb[q2][py][4 * cg]) = make_float4(s23[0].x, s23[1].x, s23[2].x, s23[3].x);
        *reinterpret_cast<float4*>(&hb[q3][py][4 * cg]) = make_float4(s23[0].y, s23[1].y, s23[2].y, s23[3].y);
    }
    __syncthreads();
    // vertical pass: column tx, rows 4 rg .. 4 rg + 3, all 8 quantities
    const int tx = tid & 31, rg = tid >> 5;
    float m[8][4];
#pragma unroll
    for (int q = 0; q < 8; q += 2) {   // two quantities per v_pk_fma_f32
        lf32x2 v[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) v[i] = (lf32x2){hb[q][4 * rg + i][tx], hb[q + 1][4 * rg + i][tx]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lf32x2 acc = (lf32x2){0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k) acc = __builtin_elementwise_fma((lf32x2){win.t[k], win.t[k]}, v[j + k], acc);
            m[q][j] = acc.x;
            m[q + 1][j] = acc.y;
        }
    }
    float ssum = 0.f;
    const long long msz = (long long)gridDim.y * Hm * Wm;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int my = my0 + 4 * rg + j, mx = mx0 + tx;
        if (!((my < Hm) && (mx < Wm))) continue;
        const float mu1 = m[0][j], mu2 = m[1][j], muf = m[2][j];
        const float sf_raw = m[5][j] - muf * muf;
        const float sf = fmaxf(sf_raw, 0.f);
        const float kf = sf_raw > 0.f ? 1.f : 0.f;
        float A = 0.f, B = 0.f, Cs[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const float mux = s2 == 0 ? mu1 : mu2;
            const float ex2 = s2 == 0 ? m[3][j] : m[4][j];
            const float exf = s2 == 0 ? m[6][j] : m[7][j];
            const float sx = fmaxf(ex2 - mux * mux, 0.f);
            // the ssim arm of ssim_pair_terms() (ssim_common.hpp), kept as this kernel's own text: it is on the train step, its code is
            // pinned instruction for instruction, and the call in its place schedules these lines differently.  Change both together.
            const float sxf = exf - mux * muf;
            const float m1 = 2.f * mux * muf + C1, m2 = mux * mux + muf * muf + C1;
            const float v1 = 2.f * sxf + C2, v2 = sx + sf + C2;
            const float inv = 1.f / (m2 * v2);
            const float S = m1 * v1 * inv;
            ssum += S;
            const float Bp = -(S / v2) * kf;
            const float Cp = 2.f * m1 * inv;
            const float Ap = 2.f * mux * v1 * inv - 2.f * muf * S / m2 - 2.f * mux * m1 * inv - 2.f * muf * Bp;
            A += Ap;
            B += Bp;
            Cs[s2] = Cp;
        }
        if (maps != nullptr) {
            const long long mi = ((long long)in_ * Hm + my) * Wm + mx;
            maps[mi] = A;
            maps[msz + mi] = B;
            maps[2 * msz + mi] = Cs[0];
            maps[3 * msz + mi] = Cs[1];
        }
    }
    const float bs = block_sum(ssum, red);
    if (tid == 0) partial[(long long)in_ * gridDim.x + blockIdx.x] = bs;
}

// ------------------------------------------------------------------ SSIM, pass 2 (adjoint correlation)
// grad[y][x] = scale * ( (G^T*mA) + 2 f (G^T*mB) + x1 (G^T*mC1) + x2 (G^T*mC2) ),
// (G^T*M)[y][x] = sum_{u,v} G[u][v] M[y-u][x-v], M zero outside the map.  Same 32 x 32 / sliding-window structure as pass 1.
__global__ __launch_bounds__(256, 2) void ssim_grad_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const float* __restrict__ f, int H, int W, SsimTaps win,
                                                           const float* __restrict__ maps, float scale,
                                                           float* __restrict__ grad, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float in[4][SIN][SPI];
    __shared__ __attribute__((aligned(16))) float hb[4][SIN][SPH];
    const int Hm = H - WIN + 1, Wm = W - WIN + 1;   // ssim_map_extent(., WIN, 0), spelled out: these two kernels' code is pinned
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % tiles_x) * ST, y0 = (blockIdx.x / tiles_x) * ST;
    const int in_ = blockIdx.y;
    const long long msz = (long long)gridDim.y * Hm * Wm;
    // map tile origin: (y0 - 10, x0 - 10)
    for (int e = tid; e < SIN * SPI; e += 256) {
        const int py = e / SPI, px = e % SPI;
        const int my = y0 - (WIN - 1) + py, mx = x0 - (WIN - 1) + px;
        const bool ok = my >= 0 && my < Hm && mx >= 0 && mx < Wm && px < SIN;
        const long long mi = ((long long)in_ * Hm + min(max(my, 0), Hm - 1)) * Wm + min(max(mx, 0), Wm - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = maps[q * msz + mi];
            in[q][py][px] = ok ? v : 0.f;
        }
    }
    __syncthreads();
    // out[x] = sum_v G[v] M[x - v]  -> with tile offset: M index px = tx + (WIN-1) - v
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        const int idx = tid + 256 * r;
        if (idx >= SIN * 8) continue;
        const int py = idx >> 3, cg = idx & 7;
#pragma unroll
        for (int q = 0; q < 4; q += 2) {   // two maps per v_pk_fma_f32
            float v0[16], v1[16];
            ld16(&in[q][py][4 * cg], v0);
            ld16(&in[q + 1][py][4 * cg], v1);
            lf32x2 v[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) v[i] = (lf32x2){v0[i], v1[i]};
            lf32x2 s2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) s2[j] = (lf32x2){0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) s2[j] = __builtin_elementwise_fma((lf32x2){win.t[k], win.t[k]}, v[j + (WIN - 1) - k], s2[j]);
            *reinterpret_cast<float4*>(&hb[q][py][4 * cg]) = make_float4(s2[0].x, s2[1].x, s2[2].x, s2[3].x);
            *reinterpret_cast<float4*>(&hb[q + 1][py][4 * cg]) = make_float4(s2[0].y, s2[1].y, s2[2].y, s2[3].y);
        }
    }
    __syncthreads();
    const int tx = tid & 31, rg = tid >> 5;
    float m[4][4];
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
        lf32x2 v[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) v[i] = (lf32x2){hb[q][4 * rg + i][tx], hb[q + 1][4 * rg + i][tx]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lf32x2 acc = (lf32x2){0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k) acc = __builtin_elementwise_fma((lf32x2){win.t[k], win.t[k]}, v[j + (WIN - 1) - k], acc);
            m[q][j] = acc.x;
            m[q + 1][j] = acc.y;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + 4 * rg + j, x = x0 + tx;
        if (y < H && x < W) {
            const long long i = ((long long)in_ * H + y) * W + x;
            grad[i] = scale * (m[0][j] + 2.f * f[i] * m[1][j] + x1[i] * m[2][j] + x2[i] * m[3][j]);
        }
    }
}

// loss = weight * (1 - 0.5 * sum / (n * nmap))
__global__ void ssim_finish_kernel(const float* __restrict__ partial, int np, float weight, float inv_count,
                                   float* __restrict__ loss) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += partial[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = weight * (1.f - 0.5f * t * inv_count);
}

// ------------------------------------------------------------------ pixel loss
// mode_max: d = f - max(x1,x2);  avg: 0.5*(|f-x1| + |f-x2|)      (core/loss.py:294-304)
__global__ __launch_bounds__(256) void pixel_loss_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ f, long long total, float gscale,
                                                         int mode_max, int l2, float* __restrict__ grad,
                                                         float* __restrict__ partial, int accum) {
    __shared__ float red[16];
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float a = x1[i], b = x2[i], c = f[i];
        float g;
        if (mode_max) {
            const float d = c - fmaxf(a, b);
            s += l2 ? d * d : fabsf(d);
            g = l2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        } else {
            const float d1 = c - a, d2 = c - b;
            s += 0.5f * (l2 ? d1 * d1 + d2 * d2 : fabsf(d1) + fabsf(d2));
            g = 0.5f * (l2 ? 2.f * (d1 + d2)
                           : ((d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f)) + (d2 > 0.f ? 1.f : (d2 < 0.f ? -1.f : 0.f))));
        }
        if (grad) grad[i] = accum ? grad[i] + gscale * g : gscale * g;   // (accum: mmif_fusion_loss adds onto the SSIM term's gradient)
    }
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void scale_finish_kernel(const float* __restrict__ partial, int np, float scale, float* __restrict__ loss) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += partial[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = scale * t;
}

// the three terms of the reference's train step (train.py:64-69) from their block partials: out = {l1 + l2 + l3, l1, l2, l3, total}.
// 1024 threads bring the partials into LDS with a few wide round trips (they were written by other XCDs: ~2 us per dependent access),
// then threads 0..255 add them in the order of the single-term finish kernels (thread t: t, t + 256, ...), so each term is
// bit-identical to its own entry point's.  Partial lists beyond the LDS budget are read directly.
constexpr int FF_CAP = 12288;   // floats of LDS staging (48 KB)
__device__ inline float ff_ordered_sum(const float* __restrict__ p, int n, float* lds) {
    const bool staged = n <= FF_CAP;
    __syncthreads();
    if (staged)
        for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = p[i];
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < 256) {
        if (staged) for (int i = threadIdx.x; i < n; i += 256) s += lds[i];
        else for (int i = threadIdx.x; i < n; i += 256) s += p[i];
    }
    return s;
}
__global__ __launch_bounds__(1024) void fusion_finish_kernel(const float* __restrict__ ps, int ns, float w_ssim, float inv_count,
                                                             const float* __restrict__ pp, int npx, float scale_px, const float* __restrict__ pg,
                                                             int ngr, float scale_gr, float* __restrict__ out) {
    __shared__ float red[16];
    __shared__ float stage[FF_CAP];
    const float ta = block_sum(ff_ordered_sum(ps, ns, stage), red);
    const float tb = block_sum(ff_ordered_sum(pp, npx, stage), red);
    const float tc = block_sum(ff_ordered_sum(pg, ngr, stage), red);
    if (threadIdx.x == 0) {
        const float l1 = w_ssim * (1.f - 0.5f * ta * inv_count), l2 = scale_px * tb, l3 = scale_gr * tc;
        out[0] = (l1 + l2) + l3;
        out[1] = l1; out[2] = l2; out[3] = l3;
        out[4] = out[0];   // (the total once more: the host side hands it out as its own 0-dim tensor)
    }
}

// ------------------------------------------------------------------ Sobel gradient loss
constexpr int GH = 3;                 // image halo in LDS
constexpr int GIN = LT + 2 * GH;      // 22
constexpr int DH = 2;                 // D-map halo in LDS
constexpr int GD = LT + 2 * DH;       // 20

__device__ inline float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// px_mode (round 6, mmif_fusion_loss only): >= 0 = this kernel also forms the PIXEL term of the same pixels (bit 0: max mode, bit 1: l2) -- its
// value as a second block partial (part_px), its gradient added between the gradient already there and the Sobel term, exactly where
// pixel_loss_kernel(accum = 1) added it: the images are in LDS here anyway, and a 9 us launch over 25 MB disappears.  -1: Sobel term only.
__global__ __launch_bounds__(256) void grad_loss_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                        const float* __restrict__ f, int H, int W, float gscale,
                                                        int mode_max, int l2, float* __restrict__ grad,
                                                        float* __restrict__ partial, int tiles_x, int accum,
                                                        int px_mode = -1, float gscale_px = 0.f, float* __restrict__ part_px = nullptr) {
    // row strides by the LDS banking of ds_read_b32 (two 32-lane groups, bank = dword index mod 32): the Sobel pass walks 20-wide rows with
    // consecutive lanes -- a stride = 20 (mod 32) keeps the 32 lanes of a group on 32 distinct banks across the row change (52 floats);
    // the adjoint pass reads 16-wide rows, two per group -- stride = 16 (mod 32) (48 floats).  (23 / 21 made every read a 2-way conflict.)
    __shared__ float in[3][GIN][52];
    __shared__ float dx[GD][48], dy[GD][48];
    __shared__ float red[16];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = (blockIdx.x % tiles_x) * LT, y0 = (blockIdx.x / tiles_x) * LT;
    const int in_ = blockIdx.y;
    const long long ibase = (long long)in_ * H * W;
    for (int e = tid; e < GIN * GIN; e += 256) {
        const int py = e / GIN, px = e % GIN;
        const int y = min(max(reflect_idx(y0 - GH + py, H), 0), H - 1);
        const int x = min(max(reflect_idx(x0 - GH + px, W), 0), W - 1);
        const long long i = ibase + (long long)y * W + x;
        in[0][py][px] = x1[i];
        in[1][py][px] = x2[i];
        in[2][py][px] = f[i];
    }
    __syncthreads();
    float lsum = 0.f;
    for (int e = tid; e < GD * GD; e += 256) {
        const int py = e / GD, px = e % GD;
        const int y = y0 - DH + py, x = x0 - DH + px;  // logical position of this D element
        float vx = 0.f, vy = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            float mag[3], sx = 0.f, sy = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                // 3x3 neighbourhood centred at LDS (py + GH - DH, px + GH - DH)
                const int cy = py + GH - DH, cx = px + GH - DH;
                const float a00 = in[q][cy - 1][cx - 1], a01 = in[q][cy - 1][cx], a02 = in[q][cy - 1][cx + 1];
                const float a10 = in[q][cy][cx - 1], a12 = in[q][cy][cx + 1];
                const float a20 = in[q][cy + 1][cx - 1], a21 = in[q][cy + 1][cx], a22 = in[q][cy + 1][cx + 1];
                const float gx = (a02 - a00) + 2.f * (a12 - a10) + (a22 - a20);
                const float gy = (a20 - a00) + 2.f * (a21 - a01) + (a22 - a02);
                mag[q] = fabsf(gx) + fabsf(gy);
                if (q == 2) { sx = sgnf(gx); sy = sgnf(gy); }
            }
            float s, l;
            if (mode_max) {
                const float d = mag[2] - fmaxf(mag[0], mag[1]);
                l = l2 ? d * d : fabsf(d);
                s = l2 ? 2.f * d : sgnf(d);
            } else {
                const float d1 = mag[2] - mag[0], d2 = mag[2] - mag[1];
                l = 0.5f * (l2 ? d1 * d1 + d2 * d2 : fabsf(d1) + fabsf(d2));
                s = 0.5f * (l2 ? 2.f * (d1 + d2) : sgnf(d1) + sgnf(d2));
            }
            vx = s * sx;
            vy = s * sy;
            // count the loss once: only positions of this block's own 16x16 tile
            if (py >= DH && py < DH + LT && px >= DH && px < DH + LT) lsum += l;
        }
        dx[py][px] = vx;
        dy[py][px] = vy;
    }
    __syncthreads();
    const int y = y0 + ty, x = x0 + tx;
    if (grad != nullptr && y < H && x < W) {
        // T(q): adjoint of the Sobel correlation on the reflect-padded domain, D zero outside the image
        auto D = [&](int qy, int qx, bool isx) -> float {
            if (qy < 0 || qy >= H || qx < 0 || qx >= W) return 0.f;
            const int ly = qy - y0 + DH, lx = qx - x0 + DH;
            return isx ? dx[ly][lx] : dy[ly][lx];
        };
        auto Tq = [&](int qy, int qx) -> float {
            // gx[p] = sum Kx[u][v] pad[p+u-1][p+v-1]  =>  T[q] = sum Kx[u][v] Dx[q-u+1][q-v+1] (+ Ky, Dy)
            float t = 0.f;
            // Kx = [[-1,0,1],[-2,0,2],[-1,0,1]]
            t += -1.f * D(qy + 1, qx + 1, true) + 1.f * D(qy + 1, qx - 1, true);
            t += -2.f * D(qy, qx + 1, true) + 2.f * D(qy, qx - 1, true);
            t += -1.f * D(qy - 1, qx + 1, true) + 1.f * D(qy - 1, qx - 1, true);
            // Ky = [[-1,-2,-1],[0,0,0],[1,2,1]]
            t += -1.f * D(qy + 1, qx + 1, false) - 2.f * D(qy + 1, qx, false) - 1.f * D(qy + 1, qx - 1, false);
            t += 1.f * D(qy - 1, qx + 1, false) + 2.f * D(qy - 1, qx, false) + 1.f * D(qy - 1, qx - 1, false);
            return t;
        };
        int ys[3], xs[3], ny = 1, nx = 1;
        ys[0] = y;
        xs[0] = x;
        if (y == 1) ys[ny++] = -1;
        if (y == H - 2) ys[ny++] = H;
        if (x == 1) xs[nx++] = -1;
        if (x == W - 2) xs[nx++] = W;
        float g = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b) g += Tq(ys[a], xs[b]);
        float* gp = grad + ibase + (long long)y * W + x;
        float base = accum ? *gp : 0.f;
        if (px_mode >= 0) {      // pixel_loss_kernel's gradient term (its arithmetic, its place in the sum)
            const float a = in[0][ty + GH][tx + GH], b = in[1][ty + GH][tx + GH], c = in[2][ty + GH][tx + GH];
            float pg;
            if (px_mode & 1) {
                const float d = c - fmaxf(a, b);
                pg = (px_mode & 2) ? 2.f * d : sgnf(d);
            } else {
                const float d1 = c - a, d2 = c - b;
                pg = 0.5f * ((px_mode & 2) ? 2.f * (d1 + d2) : sgnf(d1) + sgnf(d2));
            }
            base = base + gscale_px * pg;
        }
        *gp = (accum || px_mode >= 0) ? base + gscale * g : gscale * g;
    }
    float psum = 0.f;
    if (px_mode >= 0 && y < H && x < W) {
        const float a = in[0][ty + GH][tx + GH], b = in[1][ty + GH][tx + GH], c = in[2][ty + GH][tx + GH];
        if (px_mode & 1) {
            const float d = c - fmaxf(a, b);
            psum = (px_mode & 2) ? d * d : fabsf(d);
        } else {
            const float d1 = c - a, d2 = c - b;
            psum = 0.5f * ((px_mode & 2) ? d1 * d1 + d2 * d2 : fabsf(d1) + fabsf(d2));
        }
    }
    const float t = block_sum(lsum, red);
    if (tid == 0) partial[(long long)in_ * gridDim.x + blockIdx.x] = t;
    if (px_mode >= 0) {
        __syncthreads();
        const float tp = block_sum(psum, red);
        if (tid == 0) part_px[(long long)in_ * gridDim.x + blockIdx.x] = tp;
    }
}

// core/loss.py:24-30: the 11 taps at sigma 1.5 (pinned bit-for-bit by tests/golden/f1)
static SsimTaps window11() { return ssim_taps(WIN, ssim_loss_sigma(WIN)); }

}  // namespace mmif

using namespace mmif;

extern "C" size_t mmif_loss_workspace(int32_t n, int32_t h, int32_t w) {
    const size_t tiles = (size_t)cdiv(h, LT) * cdiv(w, LT) * n;
    const size_t maps = (size_t)4 * n * (h > 10 ? h - 10 : 0) * (w > 10 ? w - 10 : 0);
    return (tiles + 4096 + maps) * sizeof(float);
}

extern "C" int mmif_ssim_loss(const float* img1, const float* img2, const float* imgf, int32_t n, int32_t h, int32_t w,
                              float weight, float data_range, float* loss_out, float* grad_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(h >= WIN && w >= WIN, "ssim_loss: image smaller than the 11x11 window (%dx%d)", h, w);
    if (workspace_bytes < mmif_loss_workspace(n, h, w)) {
        set_error("ssim_loss: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const SsimTaps win = window11();
    const SsimConsts<float> c = ssim_consts(data_range);
    const int Hm = ssim_map_extent(h, WIN, 0), Wm = ssim_map_extent(w, WIN, 0);
    const int tmx = cdiv(Wm, ST), tmy = cdiv(Hm, ST);
    float* partial = (float*)workspace;
    const int np = tmx * tmy * n;
    float* maps = grad_out ? partial + (((size_t)np + 63) / 64) * 64 : nullptr;
    hipLaunchKernelGGL(ssim_stats_kernel, dim3(tmx * tmy, n), dim3(256), 0, st, img1, img2, imgf, h, w, win, c.C1, c.C2, maps,
                       partial, tmx);
    if (int rc = check_launch("ssim_stats")) return rc;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, st, partial, np, weight, 1.f / ((float)n * Hm * Wm),
                       loss_out);
    if (int rc = check_launch("ssim_finish")) return rc;
    if (grad_out) {
        const int tx = cdiv(w, ST), ty = cdiv(h, ST);
        const float scale = -weight * 0.5f / ((float)n * Hm * Wm);
        hipLaunchKernelGGL(ssim_grad_kernel, dim3(tx * ty, n), dim3(256), 0, st, img1, img2, imgf, h, w, win, maps, scale,
                           grad_out, tx);
        if (int rc = check_launch("ssim_grad")) return rc;
    }
    return MMIF_OK;
}

extern "C" int mmif_pixel_loss(const float* img1, const float* img2, const float* imgf, int32_t n, int32_t h, int32_t w,
                               float weight, int32_t mode_max, int32_t l2, float* loss_out, float* grad_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (workspace_bytes < mmif_loss_workspace(n, h, w)) {
        set_error("pixel_loss: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)n * h * w;
    int nb = cdiv(total, 256);
    if (nb > 2048) nb = 2048;
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(pixel_loss_kernel, dim3(nb), dim3(256), 0, st, img1, img2, imgf, total, weight / (float)total, mode_max,
                       l2, grad_out, partial, 0);
    if (int rc = check_launch("pixel_loss")) return rc;
    hipLaunchKernelGGL(scale_finish_kernel, dim3(1), dim3(256), 0, st, partial, nb, weight / (float)total, loss_out);
    return check_launch("pixel_finish");
}

extern "C" int mmif_grad_loss(const float* img1, const float* img2, const float* imgf, int32_t n, int32_t h, int32_t w,
                              float weight, int32_t mode_max, int32_t l2, float* loss_out, float* grad_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(h >= 2 && w >= 2, "grad_loss: reflect padding needs h,w >= 2");
    if (workspace_bytes < mmif_loss_workspace(n, h, w)) {
        set_error("grad_loss: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int tx = cdiv(w, LT), ty = cdiv(h, LT);
    const long long total = (long long)n * h * w;
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(grad_loss_kernel, dim3(tx * ty, n), dim3(256), 0, st, img1, img2, imgf, h, w, weight / (float)total,
                       mode_max, l2, grad_out, partial, tx, 0);
    if (int rc = check_launch("grad_loss")) return rc;
    hipLaunchKernelGGL(scale_finish_kernel, dim3(1), dim3(256), 0, st, partial, tx * ty * n, weight / (float)total, loss_out);
    return check_launch("grad_finish");
}

// SSIMLoss('ssim') + PixelLoss + GradLoss of one train step as ONE call (reference train.py:64-69: three modules, their sum, three
// gradient contributions added by autograd): the same kernels as the three calls above, the pixel and Sobel kernels adding onto the
// SSIM term's gradient, one finish kernel.  loss_out = {total, ssim, pixel, grad, total} (5 floats on the device).
static size_t fusion_parts(int32_t n, int32_t h, int32_t w, size_t* o_px, size_t* o_gr, size_t* o_maps) {
    const int Hm = ssim_map_extent(h, WIN, 0), Wm = ssim_map_extent(w, WIN, 0);
    const size_t ns = (size_t)cdiv(Wm, ST) * cdiv(Hm, ST) * n, ngr = (size_t)cdiv(w, LT) * cdiv(h, LT) * n;
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    *o_px = up(ns);
    *o_gr = *o_px + up(ngr);      // (the pixel term's partials: one per Sobel tile since round 6)
    *o_maps = *o_gr + up(ngr);
    return *o_maps + (size_t)4 * n * (h > 10 ? h - 10 : 0) * (w > 10 ? w - 10 : 0);
}
extern "C" size_t mmif_fusion_loss_workspace(int32_t n, int32_t h, int32_t w) {
    size_t a, b, c;
    return fusion_parts(n, h, w, &a, &b, &c) * sizeof(float);
}
extern "C" int mmif_fusion_loss(const float* img1, const float* img2, const float* imgf, int32_t n, int32_t h, int32_t w, float w_ssim,
                                float data_range, float w_pixel, int32_t pixel_max, int32_t pixel_l2, float w_grad, int32_t grad_max,
                                int32_t grad_l2, float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream) {
    MMIF_REQUIRE(h >= WIN && w >= WIN, "fusion_loss: image smaller than the 11x11 window (%dx%d)", h, w);
    size_t o_px, o_gr, o_maps;
    if (workspace_bytes < fusion_parts(n, h, w, &o_px, &o_gr, &o_maps) * sizeof(float)) {
        set_error("fusion_loss: workspace too small");
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const SsimTaps win = window11();
    const SsimConsts<float> c = ssim_consts(data_range);
    const int Hm = ssim_map_extent(h, WIN, 0), Wm = ssim_map_extent(w, WIN, 0);
    const int tmx = cdiv(Wm, ST), tmy = cdiv(Hm, ST);
    float* ps = (float*)workspace;
    float *pp = ps + o_px, *pg = ps + o_gr, *maps = grad_out ? ps + o_maps : nullptr;
    const int ns = tmx * tmy * n;
    hipLaunchKernelGGL(ssim_stats_kernel, dim3(tmx * tmy, n), dim3(256), 0, st, img1, img2, imgf, h, w, win, c.C1, c.C2, maps, ps, tmx);
    if (int rc = check_launch("fusion_loss ssim_stats")) return rc;
    if (grad_out) {
        const int tx = cdiv(w, ST), ty = cdiv(h, ST);
        hipLaunchKernelGGL(ssim_grad_kernel, dim3(tx * ty, n), dim3(256), 0, st, img1, img2, imgf, h, w, win, maps,
                           -w_ssim * 0.5f / ((float)n * Hm * Wm), grad_out, tx);
        if (int rc = check_launch("fusion_loss ssim_grad")) return rc;
    }
    const long long total = (long long)n * h * w;
    // the pixel term rides in the Sobel kernel (round 6): same arithmetic, its gradient added at the same place of the sum, its value from
    // 16 x 16-tile partials (mmif_pixel_loss sums grid-stride partials: equal to ~1e-7); the same kernel with and without a gradient
    const int tx = cdiv(w, LT), ty = cdiv(h, LT);
    hipLaunchKernelGGL(grad_loss_kernel, dim3(tx * ty, n), dim3(256), 0, st, img1, img2, imgf, h, w, w_grad / (float)total, grad_max, grad_l2,
                       grad_out, pg, tx, 1, (pixel_max ? 1 : 0) | (pixel_l2 ? 2 : 0), w_pixel / (float)total, pp);
    if (int rc = check_launch("fusion_loss pixel + grad")) return rc;
    hipLaunchKernelGGL(fusion_finish_kernel, dim3(1), dim3(1024), 0, st, ps, ns, w_ssim, 1.f / ((float)n * Hm * Wm), pp, tx * ty * n,
                       w_pixel / (float)total, pg, tx * ty * n, w_grad / (float)total, loss_out);
    return check_launch("fusion_loss finish");
}
