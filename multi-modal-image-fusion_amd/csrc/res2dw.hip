// Hierarchical depth-wise chain (Res2ConvBlock.dwconvs, reference core/block.py:334-340): a tensor of nseg * c channels, fp32 NCHW; segment
// i = channels [i c, (i + 1) c).  Segment 0 is a 1 x 1 depth-wise conv, every later one a 3 x 3 (stride 1, padding 1, reflect | zero), and from
// the third on a segment convolves the SUM of its own input and the previous segment's output:
//   in_0 = x_0, in_1 = x_1, in_i = y_{i-1} + x_i (i >= 2);   y_i = b_i + conv_i(pad(in_i))
// The weights are one packed buffer (segment 0 at 0 as [c], segment i >= 1 at float offset c + 9 c (i - 1) as [c][3][3]).  include/mmif.h is
// the contract.
//
//   chain     one block pass = the chain of ONE channel column (channels j, c + j, 2 c + j, ...) over one R2_TH x R2_TW tile, forward from
//             segment 1 up, input gradient from segment nseg - 1 down (G_i = gy_i + dx_{i+1}, dx_i = the adjoint of stage i on G_i).  The
//             running stage lives in LDS, in two buffers used alternately; x_i | gy_i of the tile plus its halo is read from global memory
//             once, y_i | dx_i written once, the sums in_i | G_i never leave the block.
//   halo      stage number t (of nseg - 1) is produced on the tile grown by nseg - 1 - t pixels and CLIPPED to the plane: the halo is
//             recomputed, not exchanged, and shrinks by one per stage.  Padding is resolved per stage on in-plane coordinates (row -1 of a
//             stage is row 1 of that stage's input), so every reflect target of a clipped region lies in the region grown by one, clipped.
//   bits      every output is computed by the same instruction sequence whatever block computes it (the bias, then 9 FMAs in tap order on
//             fl(y_{i-1} + x_i)): the values a block recomputes in its halo are the bits the neighbouring block stores.
//   thread    one item = a strip of R2_STRIP = 4 neighbouring outputs of one row; strips sit on multiples of 4 of the plane's columns
//             (LDS column 0 = plane column x0 - R2_XOFF), so global loads / stores and LDS writes are 16-byte accesses wherever the row is.
//   wgrad     needs no chain: with the forward's y and the input gradient's dx, segment i's operands are gy_i + dx_{i+1} and x_i + y_{i-1},
//             formed on the load.  Stage 1: 9 + 1 register accumulators per thread over its strip, wave butterfly, the 4 waves added in
//             order, one partial per (sample, tile, channel) in the workspace; stage 2: one block per channel adds the n * tiles partials
//             in a fixed order.  No atomics; the grids and every constant depend on the shape only.
#include "common.hpp"

namespace mmif {

constexpr int R2_TH = 32, R2_TW = 64, R2_STRIP = 4;
constexpr int R2_SMAX = 8;                          // segments
constexpr int R2_HALO = R2_SMAX - 1;                // the deepest input halo: x_1 | gy_{S-1} at nseg = 8
constexpr int R2_XOFF = 8;                          // LDS column 0 = plane column x0 - R2_XOFF (>= R2_HALO, a multiple of 4)
constexpr int R2_PITCH = R2_TW + 2 * R2_XOFF;       // 80
constexpr int R2_ROWS = R2_TH + 2 * R2_HALO;        // 46: two buffers of 46 x 80 floats = 28.75 KiB per block
constexpr int R2_MAX_BLOCKS = 4096;                 // every launcher walks its (column | plane, tile) list with at most this many blocks
constexpr int R2_WTH = 16, R2_WTW = 64;             // the weight gradient's tile
constexpr int R2_WPITCH = 128;                      // (csrc/mixdw.hip MD_PITCH: 16-byte LDS reads of four rows tile the 64 banks)
constexpr int R2_SLOTS = 10;                        // workspace floats per (sample, tile, channel): taps at 0 .. 8, the bias sum at 9
constexpr int R2_SUBS = 16;                         // the reduce adds a channel's partials in R2_SUBS interleaved chains, then those in order

struct R2 {
    int n, c, nseg, h, wd, reflect;
    int tiles_x, tiles_y;       // R2_TH x R2_TW tiles (forward, input gradient)
    int wtiles_x, wtiles_y;     // R2_WTH x R2_WTW tiles (weight gradient)
};

__host__ __device__ inline int r2_woff(int c, int seg) { return seg == 0 ? 0 : c + (seg - 1) * 9 * c; }

// a value that is the same in every lane, kept in a scalar register
__device__ inline float r2_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// the tile grown by g, clipped to the plane: rows [ry0, ry0 + nrows), columns [cx0, cx1) = strips [s0, s0 + nstr) (strip s = plane columns
// x0 - R2_XOFF + 4 s .. + 3)
struct R2Region {
    int ry0, nrows, cx0, cx1, s0, nstr;
};
__device__ inline R2Region r2_region(const R2& q, int y0, int x0, int g) {
    R2Region r;
    r.ry0 = max(0, y0 - g);
    r.nrows = min(q.h, y0 + R2_TH + g) - r.ry0;
    r.cx0 = max(0, x0 - g);
    r.cx1 = min(q.wd, x0 + R2_TW + g);
    r.s0 = (r.cx0 - (x0 - R2_XOFF)) >> 2;
    r.nstr = ((r.cx1 - 1 - (x0 - R2_XOFF)) >> 2) + 1 - r.s0;
    return r;
}

// four neighbouring values of row `row` from column col0 (a multiple of 4, may be negative); 0 outside the row
__device__ inline void r2_load4(const float* __restrict__ pl, int wd, int row, int col0, int vec, float (&v)[4]) {
    const float* p = pl + (long long)row * wd;
    if (vec && col0 >= 0 && col0 + 3 < wd) {
        const float4 a = *reinterpret_cast<const float4*>(p + col0);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < R2_STRIP; ++j) v[j] = (col0 + j >= 0 && col0 + j < wd) ? p[col0 + j] : 0.f;
    }
}

__device__ inline void r2_store4(float* __restrict__ pl, int wd, int row, int col0, int vec, const float (&v)[4]) {
    float* p = pl + (long long)row * wd;
    if (vec && col0 + 3 < wd) {
        *reinterpret_cast<float4*>(p + col0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < R2_STRIP; ++j)
            if (col0 + j < wd) p[col0 + j] = v[j];
    }
}

// the 3 x 6 window of the strip at (row, col0): buffer rows row - 1 .. row + 1, columns col0 - 1 .. col0 + 4.  Padding on in-plane
// coordinates: reflect folds the index, otherwise a position outside the plane is 0.  (The clamps act only on positions that no in-region
// output uses: the overhang of a clipped strip.)
__device__ inline void r2_window(const float* __restrict__ buf, const R2& q, int by0, int bx0, int row, int col0, bool reflect, float (&win)[3][6]) {
    int lrow[3], lcol[6];
    bool rok[3], cok[6];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        int t = row + u - 1;
        rok[u] = reflect || (t >= 0 && t < q.h);
        if (reflect) t = reflect_idx(t, q.h);
        lrow[u] = min(max(t - by0, 0), R2_ROWS - 1) * R2_PITCH;
    }
#pragma unroll
    for (int v = 0; v < 6; ++v) {
        int t = col0 + v - 1;
        cok[v] = reflect || (t >= 0 && t < q.wd);
        if (reflect) t = reflect_idx(t, q.wd);
        lcol[v] = min(max(t - bx0, 0), R2_PITCH - 1);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) win[u][v] = (rok[u] && cok[v]) ? buf[lrow[u] + lcol[v]] : 0.f;
}

// y = b + sum_{u,v} w[u][v] in[R(row + u - 1)][R(col + v - 1)]: the bias, then 9 FMAs in tap order
__device__ inline void r2_fwd_strip(const float* __restrict__ buf, const float (&wr)[9], float b, const R2& q, int by0, int bx0, int row, int col0,
                                    float (&acc)[4]) {
    float win[3][6];
    r2_window(buf, q, by0, bx0, row, col0, q.reflect != 0, win);
#pragma unroll
    for (int j = 0; j < R2_STRIP; ++j) acc[j] = b;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int j = 0; j < R2_STRIP; ++j) acc[j] = fmaf(wr[u * 3 + v], win[u][j + v], acc[j]);
}

// the exact adjoint of a padded 3 x 3 stage.  In-plane image: dx[y][x] = sum_{u,v} w[u][v] G[y + 1 - u][x + 1 - v] (G = 0 outside the plane), 9
// FMAs from 0.  Reflect: a pixel in row / column 1 or extent - 2 also is the target of padded position -1 / extent.  Of such an image only
// one tap row / column meets the plane: image -1 reaches G row 0 = y - 1 with tap u = 0, image h reaches G row h - 1 = y + 1 with tap u = 2 (columns
// alike), i.e. window rows 0 / 2 are used a second time with tap rows 0 / 2.  Those 16 (row pair, column pair) terms with at least one mirror are
// one more chain from 0 in a fixed order, each weight replaced by 0 where its mirror does not exist, added last.
__device__ inline void r2_dgrad_strip(const float* __restrict__ buf, const float (&wr)[9], const R2& q, int by0, int bx0, int row, int col0,
                                      float (&acc)[4]) {
    float win[3][6];
    r2_window(buf, q, by0, bx0, row, col0, false, win);
#pragma unroll
    for (int j = 0; j < R2_STRIP; ++j) acc[j] = 0.f;
    // window row a holds G row `row - 1 + a`, i.e. tap u = 2 - a; window column j + b holds G column x - 1 + b, i.e. tap v = 2 - b
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int j = 0; j < R2_STRIP; ++j) acc[j] = fmaf(wr[(2 - a) * 3 + (2 - b)], win[a][j + b], acc[j]);
    if (!q.reflect) return;
    const bool my[2] = {row == 1, row == q.h - 2};      // mirror e: window row 2 e with tap row 2 e
    const bool strip_mx = (unsigned)(1 - col0) < 4u || (unsigned)(q.wd - 2 - col0) < 4u;
    if (!(my[0] || my[1] || strip_mx)) return;
#pragma unroll
    for (int j = 0; j < R2_STRIP; ++j) {
        const bool mx[2] = {col0 + j == 1, col0 + j == q.wd - 2};
        float m = 0.f;
#pragma unroll
        for (int e = 0; e < 2; ++e)         // mirror row, in-plane column
#pragma unroll
            for (int b = 0; b < 3; ++b) m = fmaf(my[e] ? wr[2 * e * 3 + (2 - b)] : 0.f, win[2 * e][j + b], m);
#pragma unroll
        for (int a = 0; a < 3; ++a)         // in-plane row, mirror column
#pragma unroll
            for (int f = 0; f < 2; ++f) m = fmaf(mx[f] ? wr[(2 - a) * 3 + 2 * f] : 0.f, win[a][j + 2 * f], m);
#pragma unroll
        for (int e = 0; e < 2; ++e)         // mirror row, mirror column
#pragma unroll
            for (int f = 0; f < 2; ++f) m = fmaf((my[e] && mx[f]) ? wr[2 * e * 3 + 2 * f] : 0.f, win[2 * e][j + 2 * f], m);
        acc[j] += m;
    }
}

// DG = false: a = x, out = y;  DG = true: a = gy, out = dx, bias unused
template <bool DG>
__global__ __launch_bounds__(256) void res2dw_chain_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, R2 q, long long total, int vec) {
    __shared__ __attribute__((aligned(16))) float lds[2][R2_ROWS * R2_PITCH];
    const int S = q.nseg, tpp = q.tiles_x * q.tiles_y;
    const long long hw = (long long)q.h * q.wd, segstride = (long long)q.c * hw;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const long long column = t / tpp;                       // (sample, channel j of every segment)
        const int tl = (int)(t - column * tpp);
        const int smp = (int)(column / q.c), j = (int)(column - (long long)smp * q.c);
        const int y0 = (tl / q.tiles_x) * R2_TH, x0 = (tl % q.tiles_x) * R2_TW;
        const int by0 = y0 - R2_HALO, bx0 = x0 - R2_XOFF;
        const float* a0 = a + ((long long)smp * S * q.c + j) * hw;
        float* o0 = out + ((long long)smp * S * q.c + j) * hw;
        {   // segment 0: 1 x 1, feeds nothing
            const R2Region r = r2_region(q, y0, x0, 0);
            const float w0 = r2_uniform(w[j]);
            const float b0 = (!DG && bias != nullptr) ? r2_uniform(bias[j]) : 0.f;
            for (int e = threadIdx.x; e < r.nrows * r.nstr; e += 256) {
                const int rr = e / r.nstr, row = r.ry0 + rr, s = r.s0 + (e - rr * r.nstr), col0 = bx0 + R2_STRIP * s;
                float v[4], o[4];
                r2_load4(a0, q.wd, row, col0, vec, v);
#pragma unroll
                for (int jj = 0; jj < R2_STRIP; ++jj) o[jj] = DG ? w0 * v[jj] : fmaf(w0, v[jj], b0);
                r2_store4(o0, q.wd, row, col0, vec, o);
            }
        }
        if (S < 2) continue;
        __syncthreads();   // the previous pass has finished with both buffers
        {   // the first 3 x 3 stage's input on the tile grown by S - 1
            const R2Region r = r2_region(q, y0, x0, S - 1);
            const float* ap = a0 + (DG ? S - 1 : 1) * segstride;
            for (int e = threadIdx.x; e < r.nrows * r.nstr; e += 256) {
                const int rr = e / r.nstr, row = r.ry0 + rr, s = r.s0 + (e - rr * r.nstr);
                float v[4];
                r2_load4(ap, q.wd, row, bx0 + R2_STRIP * s, vec, v);
                *reinterpret_cast<float4*>(&lds[0][(row - by0) * R2_PITCH + R2_STRIP * s]) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        __syncthreads();
        int cur = 0;
        for (int st = 1; st < S; ++st) {
            const int seg = DG ? S - st : st, nxt = DG ? seg - 1 : seg + 1, g = S - 1 - st;
            const bool more = st < S - 1;
            const float* wc = w + r2_woff(q.c, seg) + j * 9;
            float wr[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) wr[k] = r2_uniform(wc[k]);
            const float b = (!DG && bias != nullptr) ? r2_uniform(bias[seg * q.c + j]) : 0.f;
            const R2Region r = r2_region(q, y0, x0, g);
            const float* buf = lds[cur];
            float* nbuf = lds[cur ^ 1];
            const float* np = a0 + nxt * segstride;
            float* op = o0 + seg * segstride;
            for (int e = threadIdx.x; e < r.nrows * r.nstr; e += 256) {
                const int rr = e / r.nstr, row = r.ry0 + rr, s = r.s0 + (e - rr * r.nstr), col0 = bx0 + R2_STRIP * s;
                float xn[4] = {0.f, 0.f, 0.f, 0.f}, acc[4];
                if (more) r2_load4(np, q.wd, row, col0, vec, xn);
                if constexpr (DG) r2_dgrad_strip(buf, wr, q, by0, bx0, row, col0, acc);
                else r2_fwd_strip(buf, wr, b, q, by0, bx0, row, col0, acc);
                if (row >= y0 && row < y0 + R2_TH && col0 >= x0 && col0 < x0 + R2_TW) r2_store4(op, q.wd, row, col0, vec, acc);
                if (more)
                    *reinterpret_cast<float4*>(&nbuf[(row - by0) * R2_PITCH + R2_STRIP * s]) =
                        make_float4(acc[0] + xn[0], acc[1] + xn[1], acc[2] + xn[2], acc[3] + xn[3]);
            }
            __syncthreads();
            cur ^= 1;
        }
    }
}

// tile[ly][lx] = B[y0 + ly - P][x0 + lx - P], B = xp (+ yp when not null), under reflect (index folded, then clamped: the clamp only acts
// on tile overhang) or zero padding
template <int K>
__device__ inline void r2_wstage(float* __restrict__ tile, const float* __restrict__ xp, const float* __restrict__ yp, int h, int wd, int y0, int x0,
                                 int reflect) {
    constexpr int P = K / 2, W = R2_WTW + 2 * P, R = R2_WTH + 2 * P;
    for (int e = threadIdx.x; e < R * W; e += 256) {
        const int ly = e / W, lx = e - ly * W;
        int gy = y0 + ly - P, gx = x0 + lx - P;
        bool ok = true;
        if (reflect) {
            gy = min(max(reflect_idx(gy, h), 0), h - 1);
            gx = min(max(reflect_idx(gx, wd), 0), wd - 1);
        } else {
            ok = gy >= 0 && gy < h && gx >= 0 && gx < wd;
        }
        float v = 0.f;
        if (ok) {
            const long long o = (long long)gy * wd + gx;
            v = yp != nullptr ? yp[o] + xp[o] : xp[o];
        }
        tile[ly * R2_WPITCH + lx] = v;
    }
}

// partial[slot] of this (sample, tile, channel): slot u K + v = sum over the tile of A B(shifted), slot R2_SLOTS - 1 = sum A; A = gp (+ dp)
template <int K>
__device__ inline void r2_wgrad_tile(float* __restrict__ tile, float* __restrict__ red, const float* __restrict__ xp, const float* __restrict__ yp,
                                     const float* __restrict__ gp, const float* __restrict__ dp, float* __restrict__ part, const R2& q, int y0, int x0) {
    r2_wstage<K>(tile, xp, yp, q.h, q.wd, y0, x0, q.reflect);
    __syncthreads();
    const int r = threadIdx.x >> 4, s = threadIdx.x & 15;
    const int oy = y0 + r, ox = x0 + R2_STRIP * s;
    float g[R2_STRIP];
#pragma unroll
    for (int j = 0; j < R2_STRIP; ++j) {
        g[j] = 0.f;
        if (oy < q.h && ox + j < q.wd) {
            const long long o = (long long)oy * q.wd + ox + j;
            g[j] = dp != nullptr ? gp[o] + dp[o] : gp[o];
        }
    }
    float acc[K * K + 1];
    acc[K * K] = ((g[0] + g[1]) + g[2]) + g[3];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        float win[8];
        const float4* qv = reinterpret_cast<const float4*>(tile + (r + u) * R2_WPITCH + R2_STRIP * s);
#pragma unroll
        for (int i = 0; i < (R2_STRIP + K - 1 + 3) / 4; ++i) {
            const float4 t4 = qv[i];
            win[4 * i] = t4.x; win[4 * i + 1] = t4.y; win[4 * i + 2] = t4.z; win[4 * i + 3] = t4.w;
        }
#pragma unroll
        for (int v = 0; v < K; ++v) {
            float t = g[0] * win[v];
#pragma unroll
            for (int j = 1; j < R2_STRIP; ++j) t = fmaf(g[j], win[j + v], t);
            acc[u * K + v] = t;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < K * K + 1; ++t) {
        float v = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave * R2_SLOTS + t] = v;
    }
    __syncthreads();
    if (threadIdx.x < K * K + 1) {
        const int t = threadIdx.x;
        const float v = ((red[t] + red[R2_SLOTS + t]) + red[2 * R2_SLOTS + t]) + red[3 * R2_SLOTS + t];
        part[t == K * K ? R2_SLOTS - 1 : t] = v;
    }
}

__global__ __launch_bounds__(256) void res2dw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                                           const float* __restrict__ dx, float* __restrict__ ws, R2 q, long long total) {
    __shared__ __attribute__((aligned(16))) float tile[(R2_WTH + 2) * R2_WPITCH];
    __shared__ float red[4 * R2_SLOTS];
    const int C = q.nseg * q.c, tpp = q.wtiles_x * q.wtiles_y;
    const long long hw = (long long)q.h * q.wd, segstride = (long long)q.c * hw;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const long long plane = t / tpp;
        const int tl = (int)(t - plane * tpp);
        const int ch = (int)(plane % C), seg = ch / q.c;
        const int y0 = (tl / q.wtiles_x) * R2_WTH, x0 = (tl % q.wtiles_x) * R2_WTW;
        const float* xp = x + plane * hw;
        const float* gp = gy + plane * hw;
        const float* yp = seg >= 2 ? y + plane * hw - segstride : nullptr;                      // in_i = x_i + y_{i-1}
        const float* dp = (seg >= 1 && seg <= q.nseg - 2) ? dx + plane * hw + segstride : nullptr;   // G_i = gy_i + dx_{i+1}
        // workspace [sample][tile][channel][R2_SLOTS]
        float* part = ws + (((plane / C) * tpp + tl) * C + ch) * R2_SLOTS;
        __syncthreads();   // the previous pass has finished with the tile
        if (seg == 0) r2_wgrad_tile<1>(tile, red, xp, yp, gp, dp, part, q, y0, x0);
        else r2_wgrad_tile<3>(tile, red, xp, yp, gp, dp, part, q, y0, x0);
    }
}

// one block per channel: thread (slot = tid & 15, sub = tid >> 4) adds entries sub, sub + 16, ... of its slot in order, then the 16 subs are
// added in order
__global__ __launch_bounds__(256) void res2dw_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, R2 q,
                                                           long long entries) {
    __shared__ float red[R2_SUBS * 16];
    const int C = q.nseg * q.c, ch = blockIdx.x, seg = ch / q.c, kk = seg == 0 ? 1 : 9;
    const int slot = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const bool live = slot < kk || slot == R2_SLOTS - 1;
    float s = 0.f;
    if (live)
        for (long long e = sub; e < entries; e += R2_SUBS) s += ws[(e * C + ch) * R2_SLOTS + slot];
    red[sub * 16 + slot] = s;
    __syncthreads();
    if (sub == 0 && live) {
        float t = red[slot];
#pragma unroll
        for (int i = 1; i < R2_SUBS; ++i) t += red[i * 16 + slot];
        if (slot < kk) dw[r2_woff(q.c, seg) + (ch - seg * q.c) * kk + slot] = t;
        else if (db != nullptr) db[ch] = t;
    }
}

static int r2_check(const char* who, int n, int c, int nseg, int h, int wd, int reflect, R2* q) {
    MMIF_REQUIRE(n > 0 && c > 0 && h > 0 && wd > 0, "%s: bad arguments (n %d, c %d, h %d, w %d)", who, n, c, h, wd);
    MMIF_REQUIRE(nseg >= 1 && nseg <= R2_SMAX, "%s: nseg must be 1..8 (got %d)", who, nseg);
    MMIF_REQUIRE(!reflect || nseg < 2 || (h >= 2 && wd >= 2), "%s: reflect padding needs h,w >= 2 (got %d x %d)", who, h, wd);
    MMIF_REQUIRE((long long)n * c * nseg * h * wd < (1ll << 31) && (long long)c * nseg <= 65535,
                 "%s: too many elements or channels (n %d, channels %lld, %d x %d)", who, n, (long long)c * nseg, h, wd);
    q->n = n; q->c = c; q->nseg = nseg; q->h = h; q->wd = wd; q->reflect = reflect ? 1 : 0;
    q->tiles_x = cdiv(wd, R2_TW); q->tiles_y = cdiv(h, R2_TH);
    q->wtiles_x = cdiv(wd, R2_WTW); q->wtiles_y = cdiv(h, R2_WTH);
    return MMIF_OK;
}

static inline long long r2_chain_total(const R2& q) { return (long long)q.n * q.c * q.tiles_x * q.tiles_y; }
static inline long long r2_wgrad_total(const R2& q) { return (long long)q.n * q.nseg * q.c * q.wtiles_x * q.wtiles_y; }
static inline int r2_grid(long long total) { return (int)(total < R2_MAX_BLOCKS ? total : R2_MAX_BLOCKS); }
static inline int r2_vec(const R2& q, const void* a, const void* b) { return (q.wd % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? 1 : 0; }

}  // namespace mmif

using namespace mmif;

extern "C" int mmif_res2dw_fwd(const float* x, const float* w, const float* bias, float* y, int32_t n, int32_t c, int32_t nseg, int32_t h, int32_t wd,
                               int32_t reflect, void* stream) {
    R2 q;
    if (int rc = r2_check("res2dw_fwd", n, c, nseg, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "res2dw_fwd: null pointer");
    const long long total = r2_chain_total(q);
    hipLaunchKernelGGL(res2dw_chain_kernel<false>, dim3(r2_grid(total)), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, q, total, r2_vec(q, x, y));
    return check_launch("res2dw_fwd");
}

extern "C" int mmif_res2dw_dgrad(const float* gy, const float* w, float* dx, int32_t n, int32_t c, int32_t nseg, int32_t h, int32_t wd, int32_t reflect,
                                 void* stream) {
    R2 q;
    if (int rc = r2_check("res2dw_dgrad", n, c, nseg, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(gy != nullptr && w != nullptr && dx != nullptr, "res2dw_dgrad: null pointer");
    const long long total = r2_chain_total(q);
    hipLaunchKernelGGL(res2dw_chain_kernel<true>, dim3(r2_grid(total)), dim3(256), 0, (hipStream_t)stream, gy, w, (const float*)nullptr, dx, q, total,
                       r2_vec(q, gy, dx));
    return check_launch("res2dw_dgrad");
}

extern "C" size_t mmif_res2dw_wgrad_workspace(int32_t n, int32_t c, int32_t nseg, int32_t h, int32_t wd) {
    R2 q;
    if (r2_check("res2dw_wgrad_workspace", n, c, nseg, h, wd, 0, &q)) return 0;
    return (size_t)r2_wgrad_total(q) * R2_SLOTS * sizeof(float);
}

extern "C" int mmif_res2dw_wgrad(const float* x, const float* y, const float* gy, const float* dx, float* dw, float* db, int32_t n, int32_t c,
                                 int32_t nseg, int32_t h, int32_t wd, int32_t reflect, void* workspace, size_t workspace_bytes, void* stream) {
    R2 q;
    if (int rc = r2_check("res2dw_wgrad", n, c, nseg, h, wd, reflect, &q)) return rc;
    MMIF_REQUIRE(x != nullptr && y != nullptr && gy != nullptr && dx != nullptr && dw != nullptr && workspace != nullptr, "res2dw_wgrad: null pointer");
    const long long total = r2_wgrad_total(q);
    const size_t need = (size_t)total * R2_SLOTS * sizeof(float);
    if (workspace_bytes < need) {
        set_error("res2dw_wgrad: workspace of %zu bytes, needs %zu", workspace_bytes, need);
        return MMIF_EWORKSPACE;
    }
    hipLaunchKernelGGL(res2dw_wgrad_kernel, dim3(r2_grid(total)), dim3(256), 0, (hipStream_t)stream, x, y, gy, dx, (float*)workspace, q, total);
    if (int rc = check_launch("res2dw_wgrad")) return rc;
    hipLaunchKernelGGL(res2dw_wgrad_reduce, dim3(q.nseg * q.c), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, db, q,
                       (long long)q.n * q.wtiles_x * q.wtiles_y);
    return check_launch("res2dw_wgrad_reduce");
}
