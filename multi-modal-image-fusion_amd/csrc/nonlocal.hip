// Res2Fusion's non-local spatial attention (reference core/fusion.py:96-113) as streaming kernels: nothing of size H*W x H*W/64 exists.
//   x [B][C][N = H*W] (plain NCHW fp32),  P = avg_pool2d(x, 8, 8) [B][C][M],  E = x^T P,  lo / hi = min / max of E over ALL of B, N, M,
//   Z = (E - lo) r,  r = 1 / (hi - lo),  S = softmax_M(Z),  y = S P + x.
// Z lies in [0, 1], so exp needs no running maximum: a streaming pass needs only the two global scalars.
//
// Every product runs on the exact fp32 matrix path (v_mfma_f32_16x16x4_f32).  One geometry serves all passes: a wave owns 16 STATIONARY
// positions (queries, or keys in the dP pass) whose features sit in registers as the B operand (lane (g = lane >> 4, n = lane & 15) holds
// channel 16 t + 4 g + u of position n for k-step (t, u)), and 16-position STREAMED tiles come through LDS in an "arranged" image
//   element (channel c, position p)  ->  row (c / 16) * 4 + (p & 3), column (p >> 2) * 16 + (c & 15)          (rows 64 wide, LDS stride 65)
// which both operand reads take without bank conflicts:
//   energy   D[p][n] = sum_c streamed[c][p] stationary[c][n]:  A of k-step (t, u) = element (16 t + 4 g + u, p = lane & 15)
//   apply    D[c][n] = sum_p streamed[c][p] W[p][n]:           A of k-step r, channel tile t = element (16 t + (lane & 15), p = 4 g + r),
//            and W is the energy tile's accumulator itself: register r of lane (g, n) is row p = 4 g + r, column n -- no lane movement.
// The apply result has channel 16 t + 4 g + r of position n in register r: the layout of the stationary registers, so "+ x" is a register add.
//
// forward : pool (P in arranged tiles) -> min/max pass (block partials, fixed-order second stage, positions recorded) -> y, l = sum exp
// backward: query-stationary pass (D, dx = g + r dZ P, T partials) -> key-stationary pass (dP partials over query chunks) -> fixed-order
//           sums -> dx += avgpool^T(dP) + the two terms routed through lo and hi.  No floating-point atomics: bit-identical run to run.
#include <float.h>

#include "common.hpp"

namespace mmif {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NL_LS = 65;        // LDS row stride of an arranged tile (64 + 1)
constexpr int NL_MAXC = 256;
constexpr int NL_SPLIT_BLOCKS = 1024;  // the dP pass splits the queries until it has about this many blocks (a constant: results do not depend on the device)
constexpr int NL_MAX_SPLIT = 64;

struct NlGeo {
    int B, C, H, W, PH, PW, KC, JT;  // KC: 16-channel tiles the kernels run; JT: 16-key tiles, rounded up to even
    long long N, M;
    long long pa_batch;              // floats of one sample's arranged P = JT * KC * 256
};

// scalar block (16 words, written by the second min/max stage, read by every later kernel)
struct NlScal {
    float lo, hi, r, pad0;
    int blo, ilo, jlo, pad1;
    int bhi, ihi, jhi, pad2;
    int pad3[4];
};

struct NlPart {  // one block's min / max and their positions (i * Mp + j)
    float mn, mx;
    long long imn, imx;
    long long pad;
};

__host__ __device__ inline long long pa_index(const NlGeo& q, int b, int c, int j) {
    return (long long)b * q.pa_batch + (long long)(j >> 4) * q.KC * 256 + ((c >> 4) * 4 + (j & 3)) * 64 + ((j & 15) >> 2) * 16 + (c & 15);
}

// ---------------------------------------------------------------- (a) pool: P, zero padded to KC * 16 channels and JT * 16 keys
__global__ void nl_pool_kernel(const float* __restrict__ x, float* __restrict__ pa, NlGeo q) {
    const long long mp = (long long)q.JT * 16, cp = q.KC * 16;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.B * cp * mp) return;
    const int j = (int)(idx % mp), c = (int)((idx / mp) % cp), b = (int)(idx / (mp * cp));
    float s = 0.f;
    if (c < q.C && j < q.M) {
        const int py = j / q.PW, px = j - py * q.PW;
        const float* src = x + ((long long)b * q.C + c) * q.N + (long long)py * 8 * q.W + px * 8;
#pragma unroll
        for (int dy = 0; dy < 8; ++dy) {
            float rs = 0.f;
#pragma unroll
            for (int dx = 0; dx < 8; ++dx) rs += src[(long long)dy * q.W + dx];
            s += rs;
        }
        s *= (1.f / 64.f);
    }
    pa[pa_index(q, b, c, j)] = s;
}

// NS energy tiles at once (independent accumulator chains): acc[s] = tile s of `lds` against the stationary registers
template <int KC, int NS>
__device__ inline void nl_energy(const float* lds, int tile_stride, const float (&st)[KC * 4], int eoff, f32x4 (&acc)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < NS; ++s)
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[s * tile_stride + eoff + t * 4 * NL_LS + u], st[t * 4 + u], acc[s], 0, 0, 0);
}

// ---------------------------------------------------------------- query-stationary passes
// MODE 0: min / max of E with positions -> part;  MODE 1: y, l;  MODE 2: backward (D, dx = g + r dZ P, T partial)
template <int KC, int NW, int MODE>
__global__ __launch_bounds__(NW * 64) void nl_query_kernel(const float* __restrict__ x, const float* __restrict__ pa, const NlScal* __restrict__ scal,
                                                           float* __restrict__ y, float* __restrict__ l, NlPart* __restrict__ part,
                                                           const float* __restrict__ gy, float* __restrict__ dx, float* __restrict__ dws,
                                                           float* __restrict__ tpart, NlGeo q) {
    extern __shared__ float smem[];
    constexpr int NT = NW * 64, TSZ = KC * 4 * NL_LS, NPF = 2 * KC * 256 / NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ii = lane & 15;
    const int b = blockIdx.y;
    const long long i0 = ((long long)blockIdx.x * NW + wave) * 16, i = i0 + ii;
    const bool qv = i < q.N, wv = i0 < q.N;
    const long long mp = (long long)q.JT * 16;
    const int eoff = (ii & 3) * NL_LS + (ii >> 2) * 16 + 4 * g;

    float xr[KC * 4], gr[MODE == 2 ? KC * 4 : 1];
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 16 * t + 4 * g + u;
            const bool ok = qv && c < q.C;
            const long long o = ((long long)b * q.C + c) * q.N + i;
            xr[t * 4 + u] = ok ? x[o] : 0.f;
            if (MODE == 2) gr[t * 4 + u] = ok ? gy[o] : 0.f;
        }
    float lo = 0.f, rr = 0.f;
    if (MODE != 0) { lo = scal->lo; rr = scal->r; }
    float dq = 0.f, linv = 0.f, tacc = 0.f;
    if (MODE == 2) {
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 16 * t + 4 * g + u;
                if (qv && c < q.C) dq += gr[t * 4 + u] * (y[((long long)b * q.C + c) * q.N + i] - xr[t * 4 + u]);
            }
        dq += __shfl_xor(dq, 16, 64);
        dq += __shfl_xor(dq, 32, 64);
        if (qv) {
            linv = 1.f / l[(long long)b * q.N + i];
            if (g == 0) dws[(long long)b * q.N + i] = dq;
        }
    }
    float mn = FLT_MAX, mx = -FLT_MAX, lsum = 0.f;
    int jmn = 0, jmx = 0;
    f32x4 oacc[MODE == 0 ? 1 : KC];
#pragma unroll
    for (int t = 0; t < (MODE == 0 ? 1 : KC); ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    float pf[NPF];
    const float* src = pa + (long long)b * q.pa_batch;
    const int npair = q.JT / 2;
    auto fetch = [&](int pair) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) pf[k] = src[(long long)pair * 2 * KC * 256 + k * NT + tid];
    };
    auto put = [&](float* dst) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int e = k * NT + tid, tile = e / (KC * 256), rem = e - tile * (KC * 256);
            dst[tile * TSZ + (rem >> 6) * NL_LS + (rem & 63)] = pf[k];
        }
    };
    fetch(0);
    put(smem);
    __syncthreads();
    for (int it = 0; it < npair; ++it) {
        const float* buf = smem + (it & 1) * 2 * TSZ;
        if (it + 1 < npair) fetch(it + 1);
        if (wv) {
            f32x4 e[2], ds[MODE == 2 ? 2 : 1];
            nl_energy<KC, 2>(buf, TSZ, xr, eoff, e);
            if constexpr (MODE == 2) nl_energy<KC, 2>(buf, TSZ, gr, eoff, ds);
            float w[2][4];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = (it * 2 + s) * 16 + 4 * g + r;
                    const bool kv = j < q.M;
                    if (MODE == 0) {
                        const float v = e[s][r];
                        if (kv && qv) {
                            if (v < mn) { mn = v; jmn = j; }
                            if (v > mx) { mx = v; jmx = j; }
                        }
                    } else {
                        const float z = (e[s][r] - lo) * rr;
                        const float p = kv ? expf(z) : 0.f;
                        if (MODE == 1) {
                            lsum += p;
                            w[s][r] = p;
                        } else {
                            const float dz = (p * linv) * (ds[s][r] - dq);
                            tacc += dz * z;
                            w[s][r] = dz;
                        }
                    }
                }
            if (MODE != 0) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int t = 0; t < KC; ++t)
                            oacc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[s * TSZ + (t * 4 + r) * NL_LS + lane], w[s][r], oacc[t], 0, 0, 0);
            }
        }
        if (it + 1 < npair) put(smem + ((it + 1) & 1) * 2 * TSZ);
        __syncthreads();
    }

    if (MODE == 0) {
        // lane -> wave -> block, ties to the smaller position: a fixed result whatever the schedule
        long long imn = qv && mn != FLT_MAX ? i * mp + jmn : LLONG_MAX, imx = qv && mx != -FLT_MAX ? i * mp + jmx : LLONG_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
            const long long oimn = __shfl_xor(imn, o, 64), oimx = __shfl_xor(imx, o, 64);
            if (omn < mn || (omn == mn && oimn < imn)) { mn = omn; imn = oimn; }
            if (omx > mx || (omx == mx && oimx < imx)) { mx = omx; imx = oimx; }
        }
        NlPart* sp = reinterpret_cast<NlPart*>(smem);  // every wave is past its last tile read (loop-end barrier)
        if (lane == 0) sp[wave] = NlPart{mn, mx, imn, imx, 0};
        __syncthreads();
        if (tid == 0) {
            NlPart a = sp[0];
            for (int k = 1; k < NW; ++k) {
                const NlPart o = sp[k];
                if (o.mn < a.mn || (o.mn == a.mn && o.imn < a.imn)) { a.mn = o.mn; a.imn = o.imn; }
                if (o.mx > a.mx || (o.mx == a.mx && o.imx < a.imx)) { a.mx = o.mx; a.imx = o.imx; }
            }
            part[(long long)b * gridDim.x + blockIdx.x] = a;
        }
        return;
    }
    if (MODE == 1) {
        lsum += __shfl_xor(lsum, 16, 64);
        lsum += __shfl_xor(lsum, 32, 64);
        const float inv = 1.f / lsum;
        if (qv) {
            if (g == 0) l[(long long)b * q.N + i] = lsum;
#pragma unroll
            for (int t = 0; t < KC; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * t + 4 * g + r;
                    if (c < q.C) y[((long long)b * q.C + c) * q.N + i] = oacc[t][r] * inv + xr[t * 4 + r];
                }
        }
        return;
    }
    if (qv) {
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * t + 4 * g + r;
                if (c < q.C) dx[((long long)b * q.C + c) * q.N + i] = gr[t * 4 + r] + rr * oacc[t][r];
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tacc += __shfl_down(tacc, o, 64);
    if (lane == 0) smem[wave] = wv ? tacc : 0.f;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int k = 0; k < NW; ++k) t += smem[k];
        tpart[(long long)b * gridDim.x + blockIdx.x] = t;
    }
}

// second min / max stage: one block, fixed order; ties go to the smaller (sample, position)
__global__ __launch_bounds__(256) void nl_minmax_final_kernel(const NlPart* __restrict__ part, int per_sample, int nparts, long long mp, NlScal* __restrict__ scal) {
    __shared__ float smn[256], smx[256];
    __shared__ long long simn[256], simx[256];
    __shared__ int sbmn[256], sbmx[256];
    float mn = FLT_MAX, mx = -FLT_MAX;
    long long imn = LLONG_MAX, imx = LLONG_MAX;
    int bmn = 0x7fffffff, bmx = 0x7fffffff;
    for (int p = threadIdx.x; p < nparts; p += 256) {
        const NlPart o = part[p];
        const int ob = p / per_sample;
        if (o.imn != LLONG_MAX && (o.mn < mn || (o.mn == mn && (ob < bmn || (ob == bmn && o.imn < imn))))) { mn = o.mn; imn = o.imn; bmn = ob; }
        if (o.imx != LLONG_MAX && (o.mx > mx || (o.mx == mx && (ob < bmx || (ob == bmx && o.imx < imx))))) { mx = o.mx; imx = o.imx; bmx = ob; }
    }
    smn[threadIdx.x] = mn; smx[threadIdx.x] = mx; simn[threadIdx.x] = imn; simx[threadIdx.x] = imx; sbmn[threadIdx.x] = bmn; sbmx[threadIdx.x] = bmx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) {
            if (smn[k] < mn || (smn[k] == mn && (sbmn[k] < bmn || (sbmn[k] == bmn && simn[k] < imn)))) { mn = smn[k]; imn = simn[k]; bmn = sbmn[k]; }
            if (smx[k] > mx || (smx[k] == mx && (sbmx[k] < bmx || (sbmx[k] == bmx && simx[k] < imx)))) { mx = smx[k]; imx = simx[k]; bmx = sbmx[k]; }
        }
        NlScal s;
        memset(&s, 0, sizeof(s));
        s.lo = mn; s.hi = mx; s.r = 1.f / (mx - mn);
        s.blo = bmn; s.ilo = (int)(imn / mp); s.jlo = (int)(imn % mp);
        s.bhi = bmx; s.ihi = (int)(imx / mp); s.jhi = (int)(imx % mp);
        *scal = s;
    }
}

// fixed-order sum of the T partials -> *t
__global__ __launch_bounds__(256) void nl_tsum_kernel(const float* __restrict__ tpart, int n, float* __restrict__ t) {
    __shared__ float s[256];
    float a = 0.f;
    for (int p = threadIdx.x; p < n; p += 256) a += tpart[p];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *t = s[0];
}

// ---------------------------------------------------------------- key-stationary pass: dP^T[c][j] = sum_i g[c][i] S[i][j] + r x[c][i] dZ[i][j]
// block = NW key tiles x one chunk of queries; x and g tiles of 32 queries are arranged into LDS on the way in
template <int KC, int NW>
__global__ __launch_bounds__(NW * 64) void nl_key_kernel(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ l,
                                                         const float* __restrict__ dws, const float* __restrict__ pa, const NlScal* __restrict__ scal,
                                                         float* __restrict__ dpp, long long qchunk, NlGeo q) {
    extern __shared__ float smem[];
    constexpr int NT = NW * 64, TSZ = KC * 4 * NL_LS, NPF = KC * 512 / NT, BUF = 4 * TSZ + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ii = lane & 15;
    const int b = blockIdx.z, split = blockIdx.y;
    const int jt = blockIdx.x * NW + wave;
    const bool wv = jt < q.JT;
    const bool kv = (long long)jt * 16 + ii < q.M;
    const long long mp = (long long)q.JT * 16;
    const int eoff = (ii & 3) * NL_LS + (ii >> 2) * 16 + 4 * g;
    const float lo = scal->lo, rr = scal->r;

    float pr[KC * 4];
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            pr[t * 4 + u] = wv ? pa[(long long)b * q.pa_batch + (long long)jt * KC * 256 + (t * 4 + (ii & 3)) * 64 + (ii >> 2) * 16 + 4 * g + u] : 0.f;
    f32x4 acc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const long long q0 = (long long)split * qchunk, q1 = min(q.N, q0 + qchunk);
    const int nit = q1 > q0 ? (int)((q1 - q0 + 31) / 32) : 0;
    float pfx[NPF], pfg[NPF], pfl = 0.f, pfd = 0.f;
    auto fetch = [&](int it) {
        const long long qb = q0 + (long long)it * 32;
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int e = k * NT + tid, c = e >> 5;
            const long long i = qb + (e & 31);
            const bool ok = c < q.C && i < q1;
            const long long o = ((long long)b * q.C + c) * q.N + i;
            pfx[k] = ok ? x[o] : 0.f;
            pfg[k] = ok ? gy[o] : 0.f;
        }
        if (tid < 32) {
            const long long i = qb + tid;
            pfl = i < q1 ? 1.f / l[(long long)b * q.N + i] : 0.f;
            pfd = i < q1 ? dws[(long long)b * q.N + i] : 0.f;
        }
    };
    auto put = [&](float* dst) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int e = k * NT + tid, c = e >> 5, qq = e & 31, iq = qq & 15;
            const int a = (qq >> 4) * TSZ + ((c >> 4) * 4 + (iq & 3)) * NL_LS + (iq >> 2) * 16 + (c & 15);
            dst[a] = pfx[k];
            dst[2 * TSZ + a] = pfg[k];
        }
        if (tid < 32) {
            dst[4 * TSZ + tid] = pfl;
            dst[4 * TSZ + 32 + tid] = pfd;
        }
    };
    if (nit > 0) {
        fetch(0);
        put(smem);
    }
    __syncthreads();
    for (int it = 0; it < nit; ++it) {
        const float* buf = smem + (it & 1) * BUF;
        if (it + 1 < nit) fetch(it + 1);
        if (wv) {
            f32x4 e[2], ds[2];
            nl_energy<KC, 2>(buf, TSZ, pr, eoff, e);
            nl_energy<KC, 2>(buf + 2 * TSZ, TSZ, pr, eoff, ds);
            float sv[2][4], dz[2][4];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int iq = s * 16 + 4 * g + r;
                    const float z = (e[s][r] - lo) * rr;
                    const float p = kv ? expf(z) : 0.f;
                    sv[s][r] = p * buf[4 * TSZ + iq];
                    dz[s][r] = rr * (sv[s][r] * (ds[s][r] - buf[4 * TSZ + 32 + iq]));
                }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int t = 0; t < KC; ++t) {
                        const int a = s * TSZ + (t * 4 + r) * NL_LS + lane;
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[2 * TSZ + a], sv[s][r], acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[a], dz[s][r], acc[t], 0, 0, 0);
                    }
        }
        if (it + 1 < nit) put(smem + ((it + 1) & 1) * BUF);
        __syncthreads();
    }
    if (wv) {
#pragma unroll
        for (int t = 0; t < KC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * t + 4 * g + r;
                dpp[(((long long)split * q.B + b) * (KC * 16) + c) * mp + (long long)jt * 16 + ii] = acc[t][r];
            }
    }
}

// dP[b][c][j] = sum of the split partials, in split order
__global__ void nl_dp_sum_kernel(const float* __restrict__ dpp, float* __restrict__ dp, int nsplit, NlGeo q) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.B * q.C * q.M) return;
    const long long j = idx % q.M, c = (idx / q.M) % q.C, b = idx / (q.M * q.C);
    const long long mp = (long long)q.JT * 16, cp = q.KC * 16;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += dpp[(((long long)k * q.B + b) * cp + c) * mp + j];
    dp[idx] = s;
}

// dx += avgpool^T(dP + the lo / hi terms of dP) + the lo / hi terms of dx   (d_lo = r T at the argmin element of E, d_hi = -r T at the argmax)
__global__ void nl_finish_kernel(const float* __restrict__ x, const float* __restrict__ pa, const float* __restrict__ dp, const NlScal* __restrict__ scal,
                                 const float* __restrict__ tsum, float* __restrict__ dx, NlGeo q) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.B * q.C * q.N) return;
    const long long n = idx % q.N;
    const int c = (int)((idx / q.N) % q.C), b = (int)(idx / (q.N * q.C));
    const int yy = (int)(n / q.W), xx = (int)(n - (long long)yy * q.W);
    const NlScal s = *scal;
    const float dlo = s.r * *tsum, dhi = -dlo;
    float v = dx[idx];
    if (yy < q.PH * 8 && xx < q.PW * 8) {
        const int j = (yy >> 3) * q.PW + (xx >> 3);
        float d = dp[((long long)b * q.C + c) * q.M + j];
        if (b == s.blo && j == s.jlo) d += dlo * x[((long long)b * q.C + c) * q.N + s.ilo];
        if (b == s.bhi && j == s.jhi) d += dhi * x[((long long)b * q.C + c) * q.N + s.ihi];
        v += d * (1.f / 64.f);
    }
    if (b == s.blo && n == s.ilo) v += dlo * pa[pa_index(q, b, c, s.jlo)];
    if (b == s.bhi && n == s.ihi) v += dhi * pa[pa_index(q, b, c, s.jhi)];
    dx[idx] = v;
}

// ---------------------------------------------------------------- host side
int kc_for(int c) {
    static const int ks[] = {1, 2, 4, 7, 8, 12, 16};
    const int need = (c + 15) / 16;
    for (int k : ks)
        if (k >= need) return k;
    return 16;
}
constexpr int nw_for(int kc) { return kc > 8 ? 4 : 8; }  // 16 queries x up to 256 channels x (x, g, dx) per lane: one wave per SIMD

bool make_geo(int n, int c, int h, int w, NlGeo& q) {
    if (n < 1 || n > 65535 || c < 1 || c > NL_MAXC || h < 8 || w < 8 || (long long)h * w > 0x3fffffffll) return false;
    q.B = n; q.C = c; q.H = h; q.W = w; q.PH = h / 8; q.PW = w / 8;
    q.N = (long long)h * w; q.M = (long long)q.PH * q.PW;
    q.KC = kc_for(c);
    q.JT = (int)((q.M + 31) / 32) * 2;
    q.pa_batch = (long long)q.JT * q.KC * 256;
    return true;
}

struct NlPlan {
    long long qblocks;        // query blocks per sample
    int kgroups, nsplit;      // dP pass: key-tile groups, query chunks
    long long qchunk;
    size_t off_pa, off_d, off_t, off_part, off_dpp, off_dp, bytes;  // workspace layout (bytes)
};

NlPlan make_plan(const NlGeo& q) {
    NlPlan p;
    const int nw = nw_for(q.KC);
    p.qblocks = (q.N + nw * 16 - 1) / (nw * 16);
    p.kgroups = (q.JT + nw - 1) / nw;
    const long long tiles32 = (q.N + 31) / 32;
    long long want = (NL_SPLIT_BLOCKS + (long long)p.kgroups * q.B - 1) / ((long long)p.kgroups * q.B);
    want = want < 1 ? 1 : (want > NL_MAX_SPLIT ? NL_MAX_SPLIT : want);
    if (want > tiles32) want = tiles32;
    p.qchunk = ((tiles32 + want - 1) / want) * 32;
    p.nsplit = (int)((q.N + p.qchunk - 1) / p.qchunk);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    p.off_pa = o;   o += up((size_t)q.B * q.pa_batch * 4);
    p.off_d = o;    o += up((size_t)q.B * q.N * 4);
    p.off_t = o;    o += 256;
    p.off_part = o; o += up((size_t)q.B * p.qblocks * sizeof(NlPart));
    p.off_dpp = o;  o += up((size_t)p.nsplit * q.B * q.KC * 16 * q.JT * 16 * 4);
    p.off_dp = o;   o += up((size_t)q.B * q.C * q.M * 4);
    p.bytes = o;
    return p;
}

template <typename K>
int raise_lds(K kernel, size_t bytes, const char* what) {
    if (bytes <= 64 * 1024) return MMIF_OK;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot raise the dynamic LDS limit to %zu bytes", what, bytes);
        return MMIF_EINVAL;
    }
    return MMIF_OK;
}

template <int KC, int MODE>
int launch_query(const float* x, const float* pa, const NlScal* scal, float* y, float* l, NlPart* part, const float* gy, float* dx, float* dws, float* tpart,
                 const NlGeo& q, const NlPlan& p, hipStream_t st) {
    constexpr int NW = nw_for(KC);
    const size_t lds = (size_t)4 * KC * 4 * NL_LS * sizeof(float);
    auto k = nl_query_kernel<KC, NW, MODE>;
    static bool raised = false;  // once per instantiation, before the first launch (and so before any capture of one)
    if (!raised) {
        if (int rc = raise_lds(k, lds, "nonlocal_spatial")) return rc;
        raised = true;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)p.qblocks, q.B), dim3(NW * 64), lds, st, x, pa, scal, y, l, part, gy, dx, dws, tpart, q);
    return check_launch(MODE == 0 ? "nonlocal_spatial minmax" : MODE == 1 ? "nonlocal_spatial fwd" : "nonlocal_spatial bwd query pass");
}

template <int KC>
int launch_key(const float* x, const float* gy, const float* l, const float* dws, const float* pa, const NlScal* scal, float* dpp, const NlGeo& q,
               const NlPlan& p, hipStream_t st) {
    constexpr int NW = nw_for(KC);
    const size_t lds = (size_t)2 * (4 * KC * 4 * NL_LS + 64) * sizeof(float);
    auto k = nl_key_kernel<KC, NW>;
    static bool raised = false;
    if (!raised) {
        if (int rc = raise_lds(k, lds, "nonlocal_spatial")) return rc;
        raised = true;
    }
    hipLaunchKernelGGL(k, dim3(p.kgroups, p.nsplit, q.B), dim3(NW * 64), lds, st, x, gy, l, dws, pa, scal, dpp, p.qchunk, q);
    return check_launch("nonlocal_spatial bwd key pass");
}

#define NL_DISPATCH(kc, CALL)                                      \
    switch (kc) {                                                  \
        case 1: { constexpr int KC = 1; CALL; } break;             \
        case 2: { constexpr int KC = 2; CALL; } break;             \
        case 4: { constexpr int KC = 4; CALL; } break;             \
        case 7: { constexpr int KC = 7; CALL; } break;             \
        case 8: { constexpr int KC = 8; CALL; } break;             \
        case 12: { constexpr int KC = 12; CALL; } break;           \
        default: { constexpr int KC = 16; CALL; } break;           \
    }

int check_args(const char* what, int n, int c, int h, int w, NlGeo& q) {
    MMIF_REQUIRE(make_geo(n, c, h, w, q), "%s: needs 1 <= n <= 65535, 1 <= c <= %d, h, w >= 8 and h * w < 2^30 (got n %d, c %d, h %d, w %d)", what, NL_MAXC, n, c, h, w);
    MMIF_REQUIRE((long long)n * c * q.N / 256 < 0x7fffffffll, "%s: n * c * h * w too large (n %d, c %d, h %d, w %d)", what, n, c, h, w);
    return MMIF_OK;
}

int run_pool(const float* x, float* pa, const NlGeo& q, hipStream_t st) {
    const long long total = (long long)q.B * q.KC * 16 * q.JT * 16;
    hipLaunchKernelGGL(nl_pool_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, x, pa, q);
    return check_launch("nonlocal_spatial pool");
}

}  // namespace
}  // namespace mmif

using namespace mmif;

extern "C" size_t mmif_nonlocal_spatial_workspace(int32_t n, int32_t c, int32_t h, int32_t w) {
    NlGeo q;
    if (check_args("mmif_nonlocal_spatial_workspace", n, c, h, w, q) != MMIF_OK) return 0;
    return make_plan(q).bytes;
}

extern "C" int mmif_nonlocal_spatial_fwd(const float* x, float* y, float* l, void* scal, int32_t n, int32_t c, int32_t h, int32_t w, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    NlGeo q;
    if (int rc = check_args("mmif_nonlocal_spatial_fwd", n, c, h, w, q)) return rc;
    MMIF_REQUIRE(x != nullptr && y != nullptr && l != nullptr && scal != nullptr && workspace != nullptr, "mmif_nonlocal_spatial_fwd: null pointer");
    const NlPlan p = make_plan(q);
    if (workspace_bytes < p.bytes) {
        set_error("mmif_nonlocal_spatial_fwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pa = (float*)(ws + p.off_pa);
    NlPart* part = (NlPart*)(ws + p.off_part);
    NlScal* sc = (NlScal*)scal;
    if (int rc = run_pool(x, pa, q, st)) return rc;
    int rc = MMIF_OK;
    NL_DISPATCH(q.KC, (rc = launch_query<KC, 0>(x, pa, sc, nullptr, nullptr, part, nullptr, nullptr, nullptr, nullptr, q, p, st)));
    if (rc) return rc;
    hipLaunchKernelGGL(nl_minmax_final_kernel, dim3(1), dim3(256), 0, st, part, (int)p.qblocks, (int)(p.qblocks * q.B), (long long)q.JT * 16, sc);
    if ((rc = check_launch("nonlocal_spatial minmax final"))) return rc;
    NL_DISPATCH(q.KC, (rc = launch_query<KC, 1>(x, pa, sc, y, l, nullptr, nullptr, nullptr, nullptr, nullptr, q, p, st)));
    return rc;
}

extern "C" int mmif_nonlocal_spatial_bwd(const float* x, const float* y, const float* l, const void* scal, const float* g, float* dx, int32_t n, int32_t c,
                                         int32_t h, int32_t w, void* workspace, size_t workspace_bytes, void* stream) {
    NlGeo q;
    if (int rc = check_args("mmif_nonlocal_spatial_bwd", n, c, h, w, q)) return rc;
    MMIF_REQUIRE(x != nullptr && y != nullptr && l != nullptr && scal != nullptr && g != nullptr && dx != nullptr && workspace != nullptr,
                 "mmif_nonlocal_spatial_bwd: null pointer");
    const NlPlan p = make_plan(q);
    if (workspace_bytes < p.bytes) {
        set_error("mmif_nonlocal_spatial_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pa = (float*)(ws + p.off_pa);
    float* dws = (float*)(ws + p.off_d);
    float* tsum = (float*)(ws + p.off_t);
    float* tpart = (float*)(ws + p.off_part);
    float* dpp = (float*)(ws + p.off_dpp);
    float* dp = (float*)(ws + p.off_dp);
    const NlScal* sc = (const NlScal*)scal;
    if (int rc = run_pool(x, pa, q, st)) return rc;
    int rc = MMIF_OK;
    NL_DISPATCH(q.KC, (rc = launch_query<KC, 2>(x, pa, sc, const_cast<float*>(y), const_cast<float*>(l), nullptr, g, dx, dws, tpart, q, p, st)));
    if (rc) return rc;
    hipLaunchKernelGGL(nl_tsum_kernel, dim3(1), dim3(256), 0, st, tpart, (int)(p.qblocks * q.B), tsum);
    if ((rc = check_launch("nonlocal_spatial T sum"))) return rc;
    NL_DISPATCH(q.KC, (rc = launch_key<KC>(x, g, l, dws, pa, sc, dpp, q, p, st)));
    if (rc) return rc;
    hipLaunchKernelGGL(nl_dp_sum_kernel, dim3((unsigned)cdiv((long long)q.B * q.C * q.M, 256)), dim3(256), 0, st, dpp, dp, p.nsplit, q);
    if ((rc = check_launch("nonlocal_spatial dP sum"))) return rc;
    hipLaunchKernelGGL(nl_finish_kernel, dim3((unsigned)cdiv((long long)q.B * q.C * q.N, 256)), dim3(256), 0, st, x, pa, dp, sc, tsum, dx, q);
    return check_launch("nonlocal_spatial finish");
}
