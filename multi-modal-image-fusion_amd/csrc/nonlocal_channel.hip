// Res2Fusion's non-local channel attention (reference core/fusion.py:137-150) and the join of attention_fusion's four maps.
//   X = x [B][C][N = H*W] (plain NCHW fp32),  E = X X^T [B][C][C],  lo / hi = min / max of E over ALL of B, C, C,
//   Z = (E - lo) r,  r = 1 / (hi - lo),  A = softmax_rows(Z),  y = A X + x.            Z lies in [0, 1]: exp needs no running maximum.
//   backward:  dA = G X^T,  D_i = sum_j dA_ij A_ij,  dZ = A o (dA - D),  T = sum dZ o Z (whole batch),
//              S = r (dZ + dZ^T) + r T at the argmin element of E and its transpose - r T at the argmax element and its transpose,
//              dx = g + A^T G + S X.
// Every product runs on the exact fp32 matrix path (v_mfma_f32_16x16x4_f32).
//
// gram    one block = (N-chunk, sample, group of 8 row tiles): 64-position tiles of X (and of G) go through LDS as [channel][position],
//         row stride 68, so that lane (g, i) reading element (16 t + i, 4 k + g) touches bank 4 i + g: both operands, no conflicts.  Wave w owns
//         row tile 8 z + w and keeps its KC column tiles in registers.  E needs the upper triangle of tiles only; the sum stage reads
//         element (min(i, j), max(i, j)) for both (i, j) and (j, i): the stored E is symmetric bit for bit.  Partials per chunk go to the
//         workspace and are summed in chunk order.
// small   sums of the partials, block min / max with positions -> one-block final stage (ties: smallest flat index of [B][C][C]) ->
//         row softmax.  Backward: one wave per row forms dA, D, dZ and the row's share of T; T is summed in a fixed order; S and A^T follow.
//         D and T are sums that cancel heavily (the rows of dZ sum to 0; sum |dZ o Z| / |T| reaches thousands) and T reaches every element of
//         dx's two routed rows, so this stage (B C^2 elements) accumulates them in double.  The routed terms themselves stay out of S: the
//         apply pass adds them to the finished products with one rounding each, instead of carrying them through the accumulator chain.
//         The stationary matrices of the apply pass are written in OPERAND order: word ((b KC + t) 4 KC + k) 64 + lane holds element
//         (16 t + (lane & 15), 4 k + (lane >> 4)), zero padded, so that a wave reads each A operand as one 256-byte line (through L2: at
//         C = 256 one matrix is 256 KiB and cannot sit in LDS).
// apply   one block = 64 positions of one sample, wave w = positions 16 w ..: X (and G) tiles in LDS as [wave][channel][16] (B operand: lane
//         (g, n) reads channel 4 k + g, position n: bank 16 g + n), KC accumulators per wave, x / g added from LDS, one store of y / dx.
// join    attention_fusion's weighted_fusion calls, clamp and mean in one element-wise launch per direction.
// No floating-point atomics anywhere: bit-identical from run to run.
#include <float.h>
#include <limits.h>

#include "common.hpp"
#include "fuse_join.hpp"

namespace mmif {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NLC_MAXC = 256;
constexpr int NLC_GS = 68;           // LDS row stride of a gram tile (64 positions + 4)
constexpr int NLC_GW = 8;            // waves (row tiles) of a gram block
constexpr int NLC_CHUNK_BLOCKS = 256;  // the gram pass cuts N into at most max(1, 256 / B) chunks per sample (a constant: results do not depend on the device)
constexpr int NLC_AW = 4;            // waves of an apply block: 64 positions
constexpr int NLC_JOIN_BLOCKS = 4096;  // grid cap of the join kernels (grid-stride beyond)

struct NlcGeo {
    int B, C, KC, CP;     // KC 16-channel tiles, CP = 16 KC padded channels
    long long N;
    long long ntiles;     // 64-position tiles
    int chunks;           // N-chunks per sample
    long long tpc;        // tiles per chunk
};

struct NlcScal {  // the scalar block of csrc/nonlocal.hip: positions are (sample, row, column) of E
    float lo, hi, r, pad0;
    int blo, ilo, jlo, pad1;
    int bhi, ihi, jhi, pad2;
    int pad3[4];
};

struct NlcPart {  // one block's min / max and their flat positions in [B][C][C]
    float mn, mx;
    long long imn, imx;
};

// ---------------------------------------------------------------- gram: part[chunk][b][row][col] = sum over the chunk's positions of A[row][p] X[col][p]
// SYM: A = X, tiles with col tile < row tile are neither computed nor stored
template <int KC, bool SYM>
__global__ __launch_bounds__(NLC_GW * 64) void nlc_gram_kernel(const float* __restrict__ x, const float* __restrict__ a, float* __restrict__ part, NlcGeo q) {
    extern __shared__ float smem[];
    constexpr int NT = NLC_GW * 64, CP = KC * 16;
    constexpr int AR = SYM ? 0 : (CP < NLC_GW * 16 ? CP : NLC_GW * 16);   // rows of the A tile held in LDS
    float* lx = smem;
    float* la = smem + CP * NLC_GS;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, ii = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the triangle test below is a branch, not a select over the accumulators)
    const int chunk = blockIdx.x, b = blockIdx.y, r0 = blockIdx.z * NLC_GW;
    const int ti = r0 + wave;
    const bool wv = ti < KC;
    f32x4 acc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long t0 = (long long)chunk * q.tpc, t1 = min(q.ntiles, t0 + q.tpc);
    const float* xb = x + (long long)b * q.C * q.N;
    const float* ab = SYM ? xb : a + (long long)b * q.C * q.N;
    const float* arow = SYM ? lx + (ti * 16 + ii) * NLC_GS + g : la + (wave * 16 + ii) * NLC_GS + g;
    for (long long tile = t0; tile < t1; ++tile) {
        const long long p0 = tile * 64;
        for (int e = tid; e < CP * 64; e += NT) {
            const int c = e >> 6, p = e & 63;
            lx[c * NLC_GS + p] = (c < q.C && p0 + p < q.N) ? xb[(long long)c * q.N + p0 + p] : 0.f;
        }
        if (!SYM) {
            for (int e = tid; e < AR * 64; e += NT) {
                const int cl = e >> 6, p = e & 63, c = r0 * 16 + cl;
                la[cl * NLC_GS + p] = (c < q.C && p0 + p < q.N) ? ab[(long long)c * q.N + p0 + p] : 0.f;
            }
        }
        __syncthreads();
        if (wv) {
#pragma unroll 2   // (unrolled further, the compiler hoists every LDS read of the tile above the MFMAs and spills at KC = 8)
            for (int k = 0; k < 16; ++k) {
                const float av = arow[4 * k];
#pragma unroll
                for (int t = 0; t < KC; ++t)
                    if (!SYM || t >= ti) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, lx[(t * 16 + ii) * NLC_GS + 4 * k + g], acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (wv) {
        float* dst = part + ((long long)chunk * q.B + b) * CP * CP;
#pragma unroll
        for (int t = 0; t < KC; ++t)
            if (!SYM || t >= ti) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[(long long)(ti * 16 + 4 * g + r) * CP + t * 16 + ii] = acc[t][r];
            }
    }
}

// ---------------------------------------------------------------- E = sum of the partials in chunk order (from the upper triangle), block min / max
__global__ __launch_bounds__(256) void nlc_esum_kernel(const float* __restrict__ part, float* __restrict__ e, NlcPart* __restrict__ mpart, NlcGeo q) {
    __shared__ NlcPart sp[256];
    const long long total = (long long)q.B * q.C * q.C;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    NlcPart m{FLT_MAX, -FLT_MAX, LLONG_MAX, LLONG_MAX};
    if (idx < total) {
        const int j = (int)(idx % q.C), i = (int)((idx / q.C) % q.C);
        const long long b = idx / ((long long)q.C * q.C);
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const long long cc = (long long)q.CP * q.CP;
        float s = 0.f;
        for (int k = 0; k < q.chunks; ++k) s += part[((long long)k * q.B + b) * cc + (long long)lo * q.CP + hi];
        e[idx] = s;
        m = NlcPart{s, s, idx, idx};
    }
    sp[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            NlcPart a = sp[threadIdx.x];
            const NlcPart c = sp[threadIdx.x + o];
            if (c.mn < a.mn || (c.mn == a.mn && c.imn < a.imn)) { a.mn = c.mn; a.imn = c.imn; }
            if (c.mx > a.mx || (c.mx == a.mx && c.imx < a.imx)) { a.mx = c.mx; a.imx = c.imx; }
            sp[threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) mpart[blockIdx.x] = sp[0];
}

// second min / max stage: one block, fixed order; ties go to the smallest flat position (sample, i C + j)
__global__ __launch_bounds__(256) void nlc_minmax_final_kernel(const NlcPart* __restrict__ mpart, long long nparts, int c, NlcScal* __restrict__ scal) {
    __shared__ NlcPart sp[256];
    NlcPart a{FLT_MAX, -FLT_MAX, LLONG_MAX, LLONG_MAX};
    for (long long p = threadIdx.x; p < nparts; p += 256) {
        const NlcPart o = mpart[p];
        if (o.imn != LLONG_MAX && (o.mn < a.mn || (o.mn == a.mn && o.imn < a.imn))) { a.mn = o.mn; a.imn = o.imn; }
        if (o.imx != LLONG_MAX && (o.mx > a.mx || (o.mx == a.mx && o.imx < a.imx))) { a.mx = o.mx; a.imx = o.imx; }
    }
    sp[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) {
            const NlcPart o = sp[k];
            if (o.imn != LLONG_MAX && (o.mn < a.mn || (o.mn == a.mn && o.imn < a.imn))) { a.mn = o.mn; a.imn = o.imn; }
            if (o.imx != LLONG_MAX && (o.mx > a.mx || (o.mx == a.mx && o.imx < a.imx))) { a.mx = o.mx; a.imx = o.imx; }
        }
        const long long cc = (long long)c * c;
        NlcScal s;
        memset(&s, 0, sizeof(s));
        s.lo = a.mn; s.hi = a.mx; s.r = 1.f / (a.mx - a.mn);
        s.blo = (int)(a.imn / cc); s.ilo = (int)((a.imn % cc) / c); s.jlo = (int)(a.imn % c);
        s.bhi = (int)(a.imx / cc); s.ihi = (int)((a.imx % cc) / c); s.jhi = (int)(a.imx % c);
        *scal = s;
    }
}

__device__ inline long long nlc_arr_index(const NlcGeo& q, long long b, int row, int col) {  // operand order of element (row, col) of a stationary matrix
    return (((b * q.KC + (row >> 4)) * (4 * q.KC) + (col >> 2)) * 64) + (col & 3) * 16 + (row & 15);
}

__device__ inline double nlc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline float nlc_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// row softmax: one wave per padded row (b, i); attn [B][C][C] and the same matrix in operand order (zero padded)
__global__ __launch_bounds__(256) void nlc_softmax_kernel(const float* __restrict__ e, const NlcScal* __restrict__ scal, float* __restrict__ attn,
                                                          float* __restrict__ arr, NlcGeo q) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)q.B * q.CP) return;
    const long long b = row / q.CP;
    const int i = (int)(row % q.CP);
    const float lo = scal->lo, rr = scal->r;
    float p[4], s = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = lane + 64 * m;
        p[m] = (i < q.C && j < q.C) ? expf((e[(b * q.C + i) * q.C + j] - lo) * rr) : 0.f;
        s += p[m];
    }
    s = nlc_wave_sum(s);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = lane + 64 * m;
        if (j >= q.CP) continue;
        const float v = (i < q.C && j < q.C) ? p[m] / s : 0.f;
        if (i < q.C && j < q.C) attn[(b * q.C + i) * q.C + j] = v;
        arr[nlc_arr_index(q, b, i, j)] = v;
    }
}

// backward rows: dA (sum of the partials in chunk order), D, dZ -> dz [B][C][C]; the row's sum dZ o Z -> tpart[b C + i]
__global__ __launch_bounds__(256) void nlc_dz_kernel(const float* __restrict__ part, const float* __restrict__ e, const float* __restrict__ attn,
                                                     const NlcScal* __restrict__ scal, float* __restrict__ dz, double* __restrict__ tpart, NlcGeo q) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)q.B * q.C) return;
    const long long b = row / q.C;
    const int i = (int)(row % q.C);
    const float lo = scal->lo, rr = scal->r;
    const long long cc = (long long)q.CP * q.CP;
    float da[4], av[4];
    double d = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = lane + 64 * m;
        da[m] = 0.f;
        av[m] = 0.f;
        if (j < q.C) {
            float s = 0.f;
            for (int k = 0; k < q.chunks; ++k) s += part[((long long)k * q.B + b) * cc + (long long)i * q.CP + j];
            da[m] = s;
            av[m] = attn[row * q.C + j];
        }
        d += (double)da[m] * av[m];
    }
    d = nlc_wave_sum(d);
    double t = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = lane + 64 * m;
        if (j < q.C) {
            const double v = av[m] * (da[m] - d);
            dz[row * q.C + j] = (float)v;
            t += v * (((double)e[row * q.C + j] - lo) * rr);
        }
    }
    t = nlc_wave_sum(t);
    if (lane == 0) tpart[row] = t;
}

// fixed-order sum of the T partials -> *t
__global__ __launch_bounds__(256) void nlc_tsum_kernel(const double* __restrict__ tpart, long long n, double* __restrict__ t) {
    __shared__ double s[256];
    double a = 0.0;
    for (long long p = threadIdx.x; p < n; p += 256) a += tpart[p];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *t = s[0];
}

// the two stationary matrices of the backward apply pass, in operand order: at (row c, col k) = A[k][c];  sm (c, k) = r (dZ[c][k] + dZ[k][c])
__global__ __launch_bounds__(256) void nlc_sym_kernel(const float* __restrict__ attn, const float* __restrict__ dz, const NlcScal* __restrict__ scal,
                                                      float* __restrict__ at, float* __restrict__ sm, NlcGeo q) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)q.B * q.CP * q.CP) return;
    const int k = (int)(idx % q.CP), c = (int)((idx / q.CP) % q.CP);
    const long long b = idx / ((long long)q.CP * q.CP);
    float va = 0.f, vs = 0.f;
    if (c < q.C && k < q.C) {
        const float rr = scal->r;
        va = attn[(b * q.C + k) * q.C + c];
        vs = rr * dz[(b * q.C + c) * q.C + k] + rr * dz[(b * q.C + k) * q.C + c];
    }
    const long long o = nlc_arr_index(q, b, c, k);
    at[o] = va;
    sm[o] = vs;
}

// ---------------------------------------------------------------- apply: out = x0 + M1 X0 (+ M2 X1 + routed);  forward (x0 = x, M1 = A), backward (x0 = g, M1 = A^T,
// M2 = S, X1 = x; routed: + r T x[jlo] in row ilo, + r T x[ilo] in row jlo of sample blo, the same with - r T for the maximum)
template <int KC, bool BWD>
__global__ __launch_bounds__(NLC_AW * 64) void nlc_apply_kernel(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ m1,
                                                                const float* __restrict__ m2, const NlcScal* __restrict__ scal, const double* __restrict__ tsum,
                                                                float* __restrict__ out, NlcGeo q) {
    extern __shared__ float smem[];
    constexpr int NT = NLC_AW * 64, CP = KC * 16, WS = CP * 16 + 16;   // WS: one wave's [channel][16] image (+ 16: the four waves start 16 banks apart)
    float* l0 = smem;
    float* l1 = smem + NLC_AW * WS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
    const long long b = blockIdx.y, p0 = (long long)blockIdx.x * 64;
    const float* s0 = x0 + b * q.C * q.N;
    const float* s1 = BWD ? x1 + b * q.C * q.N : nullptr;
    for (int e = tid; e < CP * 64; e += NT) {
        const int c = e >> 6, p = e & 63;
        const bool ok = c < q.C && p0 + p < q.N;
        const int a = (p >> 4) * WS + c * 16 + (p & 15);
        l0[a] = ok ? s0[(long long)c * q.N + p0 + p] : 0.f;
        if (BWD) l1[a] = ok ? s1[(long long)c * q.N + p0 + p] : 0.f;
    }
    __syncthreads();
    const long long pw = p0 + wave * 16;
    if (pw >= q.N) return;
    f32x4 acc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* w0 = l0 + wave * WS + g * 16 + n;
    const float* w1 = l1 + wave * WS + g * 16 + n;
    const float* a1 = m1 + b * CP * CP + lane;
    const float* a2 = BWD ? m2 + b * CP * CP + lane : nullptr;
#pragma unroll 2
    for (int k = 0; k < 4 * KC; ++k) {
        const float b0 = w0[k * 64];
        const float b1 = BWD ? w1[k * 64] : 0.f;
#pragma unroll
        for (int t = 0; t < KC; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[(t * 4 * KC + k) * 64], b0, acc[t], 0, 0, 0);
            if (BWD) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[(t * 4 * KC + k) * 64], b1, acc[t], 0, 0, 0);
        }
    }
    if (pw + n < q.N) {
        float* dst = out + b * q.C * q.N + pw + n;
        NlcScal s;
        float rt = 0.f;
        const float* xw = l1 + wave * WS + n;   // x of this lane's position, by channel
        if (BWD) {
            s = *scal;
            rt = (float)((double)s.r * *tsum);
        }
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = t * 16 + 4 * g + r;
                if (c >= q.C) continue;
                float d = acc[t][r];
                if (BWD) {
                    if (b == s.blo) {
                        if (c == s.ilo) d += rt * xw[s.jlo * 16];
                        if (c == s.jlo) d += rt * xw[s.ilo * 16];
                    }
                    if (b == s.bhi) {
                        if (c == s.ihi) d -= rt * xw[s.jhi * 16];
                        if (c == s.jhi) d -= rt * xw[s.ihi * 16];
                    }
                }
                dst[(long long)c * q.N] = l0[wave * WS + c * 16 + n] + d;
            }
    }
}

// ---------------------------------------------------------------- the join (attention_fusion core/fusion.py:42-59 with both poolings 'nl')
// Wf, wf_fwd, wf_bwd: fuse_join.hpp (shared with csrc/attn_fuse.hip)
// mode 0 'sa', 1 'ca', 2 'sca', 3 'wavg'
template <int MODE>
__global__ __launch_bounds__(256) void join_fwd_kernel(const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ s1,
                                                       const float* __restrict__ s2, const float* __restrict__ c1, const float* __restrict__ c2,
                                                       float* __restrict__ out, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const float a = t1[i], b = t2[i];
        float fs = 0.f, fc = 0.f;
        if (MODE != 1) fs = wf_fwd(a, b, s1[i], s2[i]).f;
        if (MODE != 0) fc = wf_fwd(a, b, c1[i], c2[i]).f;
        float o;
        if (MODE == 0) o = fs;
        else if (MODE == 1) o = fc;
        else if (MODE == 2) o = (fs + fc) / 2.0f;
        else o = wf_fwd(fs, fc, fs, fc).f;
        out[i] = o;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void join_bwd_kernel(const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ s1,
                                                       const float* __restrict__ s2, const float* __restrict__ c1, const float* __restrict__ c2,
                                                       const float* __restrict__ g, float* __restrict__ dt1, float* __restrict__ dt2,
                                                       float* __restrict__ ds1, float* __restrict__ ds2, float* __restrict__ dc1,
                                                       float* __restrict__ dc2, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const float a = t1[i], b = t2[i], gi = g[i];
        Wf ws{}, wc{};
        if (MODE != 1) ws = wf_fwd(a, b, s1[i], s2[i]);
        if (MODE != 0) wc = wf_fwd(a, b, c1[i], c2[i]);
        float dfs = 0.f, dfc = 0.f;
        if (MODE == 0) dfs = gi;
        else if (MODE == 1) dfc = gi;
        else if (MODE == 2) { dfs = gi / 2.0f; dfc = dfs; }
        else {  // out = wf(fs, fc, fs, fc): fs and fc are both operands and weights
            const Wf wo = wf_fwd(ws.f, wc.f, ws.f, wc.f);
            float da, db;
            wf_bwd(wo, ws.f, wc.f, gi, da, db);
            dfs = gi * wo.w + da;
            dfc = gi * (1.f - wo.w) + db;
        }
        float d1 = 0.f, d2 = 0.f;
        if (MODE != 1) {
            float da, db;
            wf_bwd(ws, a, b, dfs, da, db);
            ds1[i] = da;
            ds2[i] = db;
            d1 += dfs * ws.w;
            d2 += dfs * (1.f - ws.w);
        }
        if (MODE != 0) {
            float da, db;
            wf_bwd(wc, a, b, dfc, da, db);
            dc1[i] = da;
            dc2[i] = db;
            d1 += dfc * wc.w;
            d2 += dfc * (1.f - wc.w);
        }
        dt1[i] = d1;
        dt2[i] = d2;
    }
}

// ---------------------------------------------------------------- host side
int nlc_kc_for(int c) {  // the widths csrc/nonlocal.hip instantiates
    static const int ks[] = {1, 2, 4, 7, 8, 12, 16};
    const int need = (c + 15) / 16;
    for (int k : ks)
        if (k >= need) return k;
    return 16;
}

bool nlc_make_geo(int n, int c, int h, int w, NlcGeo& q) {
    if (n < 1 || n > 65535 || c < 1 || c > NLC_MAXC || h < 1 || w < 1 || (long long)h * w > 0x3fffffffll || (long long)n * c < 2) return false;
    q.B = n; q.C = c; q.KC = nlc_kc_for(c); q.CP = q.KC * 16;
    q.N = (long long)h * w;
    q.ntiles = (q.N + 63) / 64;
    long long cap = NLC_CHUNK_BLOCKS / n;
    if (cap < 1) cap = 1;
    const long long want = q.ntiles < cap ? q.ntiles : cap;
    q.tpc = (q.ntiles + want - 1) / want;
    q.chunks = (int)((q.ntiles + q.tpc - 1) / q.tpc);
    return true;
}

struct NlcPlan {
    long long eblocks;   // blocks of the E-sum stage = min / max partials
    size_t off_part, off_arr1, off_arr2, off_dz, off_mpart, off_tpart, off_t, bytes;
};

NlcPlan nlc_make_plan(const NlcGeo& q) {
    NlcPlan p;
    p.eblocks = ((long long)q.B * q.C * q.C + 255) / 256;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t mat = (size_t)q.B * q.CP * q.CP * 4;
    size_t o = 0;
    p.off_part = o;  o += up((size_t)q.chunks * mat);
    p.off_arr1 = o;  o += up(mat);
    p.off_arr2 = o;  o += up(mat);
    p.off_dz = o;    o += up((size_t)q.B * q.C * q.C * 4);
    p.off_mpart = o; o += up((size_t)p.eblocks * sizeof(NlcPart));
    p.off_tpart = o; o += up((size_t)q.B * q.C * sizeof(double));
    p.off_t = o;     o += 256;
    p.bytes = o;
    return p;
}

template <typename K>
int nlc_raise_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return MMIF_OK;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("nonlocal_channel: cannot raise the dynamic LDS limit to %zu bytes", bytes);
        return MMIF_EINVAL;
    }
    return MMIF_OK;
}

template <int KC, bool SYM>
int launch_gram(const float* x, const float* a, float* part, const NlcGeo& q, hipStream_t st) {
    constexpr int CP = KC * 16, AR = SYM ? 0 : (CP < NLC_GW * 16 ? CP : NLC_GW * 16);
    const size_t lds = (size_t)(CP + AR) * NLC_GS * sizeof(float);
    auto k = nlc_gram_kernel<KC, SYM>;
    static bool raised = false;  // once per instantiation, before the first launch (and so before any capture of one)
    if (!raised) {
        if (int rc = nlc_raise_lds(k, lds)) return rc;
        raised = true;
    }
    hipLaunchKernelGGL(k, dim3(q.chunks, q.B, (KC + NLC_GW - 1) / NLC_GW), dim3(NLC_GW * 64), lds, st, x, a, part, q);
    return check_launch(SYM ? "nonlocal_channel energy" : "nonlocal_channel bwd dA");
}

template <int KC, bool BWD>
int launch_apply(const float* x0, const float* x1, const float* m1, const float* m2, const NlcScal* scal, const double* tsum, float* out, const NlcGeo& q,
                 hipStream_t st) {
    const size_t lds = (size_t)(BWD ? 2 : 1) * NLC_AW * (KC * 256 + 16) * sizeof(float);
    auto k = nlc_apply_kernel<KC, BWD>;
    static bool raised = false;
    if (!raised) {
        if (int rc = nlc_raise_lds(k, lds)) return rc;
        raised = true;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)q.ntiles, q.B), dim3(NLC_AW * 64), lds, st, x0, x1, m1, m2, scal, tsum, out, q);
    return check_launch(BWD ? "nonlocal_channel bwd apply" : "nonlocal_channel fwd apply");
}

#define NLC_DISPATCH(kc, CALL)                                     \
    switch (kc) {                                                  \
        case 1: { constexpr int KC = 1; CALL; } break;             \
        case 2: { constexpr int KC = 2; CALL; } break;             \
        case 4: { constexpr int KC = 4; CALL; } break;             \
        case 7: { constexpr int KC = 7; CALL; } break;             \
        case 8: { constexpr int KC = 8; CALL; } break;             \
        case 12: { constexpr int KC = 12; CALL; } break;           \
        default: { constexpr int KC = 16; CALL; } break;           \
    }

int nlc_check_args(const char* what, int n, int c, int h, int w, NlcGeo& q) {
    MMIF_REQUIRE(nlc_make_geo(n, c, h, w, q), "%s: needs 1 <= n <= 65535, 1 <= c <= %d, n * c >= 2, h, w >= 1 and h * w < 2^30 (got n %d, c %d, h %d, w %d)", what,
                 NLC_MAXC, n, c, h, w);
    return MMIF_OK;
}

int join_check(const char* what, const float* t1, const float* t2, const float* s1, const float* s2, const float* c1, const float* c2, int32_t mode,
               size_t count) {
    MMIF_REQUIRE(mode >= 0 && mode <= 3, "%s: mode %d (0 'sa', 1 'ca', 2 'sca', 3 'wavg')", what, mode);
    MMIF_REQUIRE(count >= 1, "%s: count 0", what);
    MMIF_REQUIRE(t1 != nullptr && t2 != nullptr, "%s: null tensor", what);
    const bool sp = mode != 1, ch = mode != 0;
    MMIF_REQUIRE((s1 != nullptr) == sp && (s2 != nullptr) == sp, "%s: mode %d %s the spatial maps", what, mode, sp ? "needs" : "takes no");
    MMIF_REQUIRE((c1 != nullptr) == ch && (c2 != nullptr) == ch, "%s: mode %d %s the channel maps", what, mode, ch ? "needs" : "takes no");
    return MMIF_OK;
}

unsigned join_grid(size_t count) {
    const size_t blocks = (count + 255) / 256;
    return (unsigned)(blocks < (size_t)NLC_JOIN_BLOCKS ? blocks : (size_t)NLC_JOIN_BLOCKS);
}

}  // namespace
}  // namespace mmif

using namespace mmif;

extern "C" size_t mmif_nonlocal_channel_workspace(int32_t n, int32_t c, int32_t h, int32_t w) {
    NlcGeo q;
    if (nlc_check_args("mmif_nonlocal_channel_workspace", n, c, h, w, q) != MMIF_OK) return 0;
    return nlc_make_plan(q).bytes;
}

extern "C" int mmif_nonlocal_channel_fwd(const float* x, float* y, float* e, float* attn, void* scal, int32_t n, int32_t c, int32_t h, int32_t w,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    NlcGeo q;
    if (int rc = nlc_check_args("mmif_nonlocal_channel_fwd", n, c, h, w, q)) return rc;
    MMIF_REQUIRE(x != nullptr && y != nullptr && e != nullptr && attn != nullptr && scal != nullptr && workspace != nullptr,
                 "mmif_nonlocal_channel_fwd: null pointer");
    const NlcPlan p = nlc_make_plan(q);
    if (workspace_bytes < p.bytes) {
        set_error("mmif_nonlocal_channel_fwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* part = (float*)(ws + p.off_part);
    float* arr = (float*)(ws + p.off_arr1);
    NlcPart* mpart = (NlcPart*)(ws + p.off_mpart);
    NlcScal* sc = (NlcScal*)scal;
    int rc = MMIF_OK;
    NLC_DISPATCH(q.KC, (rc = launch_gram<KC, true>(x, nullptr, part, q, st)));
    if (rc) return rc;
    hipLaunchKernelGGL(nlc_esum_kernel, dim3((unsigned)p.eblocks), dim3(256), 0, st, part, e, mpart, q);
    if ((rc = check_launch("nonlocal_channel energy sum"))) return rc;
    hipLaunchKernelGGL(nlc_minmax_final_kernel, dim3(1), dim3(256), 0, st, mpart, p.eblocks, q.C, sc);
    if ((rc = check_launch("nonlocal_channel minmax final"))) return rc;
    hipLaunchKernelGGL(nlc_softmax_kernel, dim3((unsigned)cdiv((long long)q.B * q.CP, 4)), dim3(256), 0, st, e, sc, attn, arr, q);
    if ((rc = check_launch("nonlocal_channel softmax"))) return rc;
    NLC_DISPATCH(q.KC, (rc = launch_apply<KC, false>(x, nullptr, arr, nullptr, nullptr, nullptr, y, q, st)));
    return rc;
}

extern "C" int mmif_nonlocal_channel_bwd(const float* x, const float* e, const float* attn, const void* scal, const float* g, float* dx, int32_t n,
                                         int32_t c, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream) {
    NlcGeo q;
    if (int rc = nlc_check_args("mmif_nonlocal_channel_bwd", n, c, h, w, q)) return rc;
    MMIF_REQUIRE(x != nullptr && e != nullptr && attn != nullptr && scal != nullptr && g != nullptr && dx != nullptr && workspace != nullptr,
                 "mmif_nonlocal_channel_bwd: null pointer");
    const NlcPlan p = nlc_make_plan(q);
    if (workspace_bytes < p.bytes) {
        set_error("mmif_nonlocal_channel_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* part = (float*)(ws + p.off_part);
    float* at = (float*)(ws + p.off_arr1);
    float* sm = (float*)(ws + p.off_arr2);
    float* dz = (float*)(ws + p.off_dz);
    double* tpart = (double*)(ws + p.off_tpart);
    double* tsum = (double*)(ws + p.off_t);
    const NlcScal* sc = (const NlcScal*)scal;
    int rc = MMIF_OK;
    NLC_DISPATCH(q.KC, (rc = launch_gram<KC, false>(x, g, part, q, st)));
    if (rc) return rc;
    hipLaunchKernelGGL(nlc_dz_kernel, dim3((unsigned)cdiv((long long)q.B * q.C, 4)), dim3(256), 0, st, part, e, attn, sc, dz, tpart, q);
    if ((rc = check_launch("nonlocal_channel bwd dZ"))) return rc;
    hipLaunchKernelGGL(nlc_tsum_kernel, dim3(1), dim3(256), 0, st, tpart, (long long)q.B * q.C, tsum);
    if ((rc = check_launch("nonlocal_channel T sum"))) return rc;
    hipLaunchKernelGGL(nlc_sym_kernel, dim3((unsigned)cdiv((long long)q.B * q.CP * q.CP, 256)), dim3(256), 0, st, attn, dz, sc, at, sm, q);
    if ((rc = check_launch("nonlocal_channel bwd matrices"))) return rc;
    NLC_DISPATCH(q.KC, (rc = launch_apply<KC, true>(g, x, at, sm, sc, tsum, dx, q, st)));
    return rc;
}

extern "C" int mmif_fuse_join_fwd(const float* t1, const float* t2, const float* s1, const float* s2, const float* c1, const float* c2, float* out,
                                  int32_t mode, size_t count, void* stream) {
    if (int rc = join_check("mmif_fuse_join_fwd", t1, t2, s1, s2, c1, c2, mode, count)) return rc;
    MMIF_REQUIRE(out != nullptr, "mmif_fuse_join_fwd: null output");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(join_grid(count)), block(256);
    switch (mode) {
        case 0: hipLaunchKernelGGL(join_fwd_kernel<0>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, out, count); break;
        case 1: hipLaunchKernelGGL(join_fwd_kernel<1>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, out, count); break;
        case 2: hipLaunchKernelGGL(join_fwd_kernel<2>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, out, count); break;
        default: hipLaunchKernelGGL(join_fwd_kernel<3>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, out, count); break;
    }
    return check_launch("fuse_join_fwd");
}

extern "C" int mmif_fuse_join_bwd(const float* t1, const float* t2, const float* s1, const float* s2, const float* c1, const float* c2, const float* g,
                                  float* dt1, float* dt2, float* ds1, float* ds2, float* dc1, float* dc2, int32_t mode, size_t count, void* stream) {
    if (int rc = join_check("mmif_fuse_join_bwd", t1, t2, s1, s2, c1, c2, mode, count)) return rc;
    MMIF_REQUIRE(g != nullptr && dt1 != nullptr && dt2 != nullptr, "mmif_fuse_join_bwd: null pointer");
    const bool sp = mode != 1, ch = mode != 0;
    MMIF_REQUIRE((ds1 != nullptr) == sp && (ds2 != nullptr) == sp && (dc1 != nullptr) == ch && (dc2 != nullptr) == ch,
                 "mmif_fuse_join_bwd: mode %d takes gradients for exactly the maps it uses", mode);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(join_grid(count)), block(256);
    switch (mode) {
        case 0: hipLaunchKernelGGL(join_bwd_kernel<0>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, g, dt1, dt2, ds1, ds2, dc1, dc2, count); break;
        case 1: hipLaunchKernelGGL(join_bwd_kernel<1>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, g, dt1, dt2, ds1, ds2, dc1, dc2, count); break;
        case 2: hipLaunchKernelGGL(join_bwd_kernel<2>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, g, dt1, dt2, ds1, ds2, dc1, dc2, count); break;
        default: hipLaunchKernelGGL(join_bwd_kernel<3>, grid, block, 0, st, t1, t2, s1, s2, c1, c2, g, dt1, dt2, ds1, ds2, dc1, dc2, count); break;
    }
    return check_launch("fuse_join_bwd");
}
