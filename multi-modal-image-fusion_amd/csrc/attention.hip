// Multi-head spatial-reduction self-attention core (reference core/block.py:416-431) as streaming kernels: nothing of size N x M exists.
//   q [B][A][N], k, v [B][A][M] (plain NCHW fp32 planes, A = heads * d, head h owns channels h d ... (h + 1) d - 1),
//   o[b][h d + c][i] = sum_j softmax_j(scale sum_c' q[c'][i] k[c'][j]) v[c][j],   lse[b][h][i] = log sum_j exp(scale q_i . k_j).
// M is any number >= 1 (not tied to N); d is 8, 16 or 32; A <= 256.
//
// Every product runs on the exact fp32 matrix path (v_mfma_f32_16x16x4_f32), in the geometry of nonlocal.hip: a wave owns 16 STATIONARY
// positions whose head features sit in registers as the B operand (lane (g = lane >> 4, n = lane & 15) holds channel 16 t + 4 g + u of
// position n for k-step (t, u)); STREAMED positions come through LDS 64 at a time as four 16-position tiles [channel][16], row stride 20:
//   score   D[p][n] = sum_c streamed[c][p] stationary[c][n]:  A of k-step (t, u) = element (16 t + 4 g + u, p = lane & 15)   (one word:
//           the four g groups are 80 words apart, so the 64 lanes touch 64 different banks)
//   apply   D[c][n] = sum_p streamed[c][p] W[p][n]:           A of k-step r, channel tile t = element (16 t + (lane & 15), p = 4 g + r):
//           four consecutive words, read as one 16-byte access; W is the score tile's accumulator itself (register r of lane (g, n)
//           is row p = 4 g + r, column n) -- no lane movement.
// The apply result has channel 16 t + 4 g + r of position n in register r: the layout of the stationary registers and of the NCHW planes.
//
// Softmax: logits are unbounded, so the forward keeps a RUNNING maximum per query and rescales the accumulator and the row sum once per
// 64-key chunk (one pass over k and v; a separate maximum pass would compute every score twice).  A key beyond M has logit -inf: weight
// exactly 0.  The backward recomputes the weights as exp(scale s - lse).
//
// backward: query-stationary pass (D = sum_c go o, dq) -> key-stationary pass (dk, dv partials over query chunks; the number of chunks
//           comes from the constant SRA_SPLIT_BLOCKS, not from the device) -> fixed-order sum.  No floating-point atomics: bit-identical
//           run to run.
#include <math.h>

#include "common.hpp"

namespace mmif {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SRA_LS = 20;             // LDS row stride of a 16-position tile
constexpr int SRA_CH = 4;              // 16-position tiles per streamed chunk
constexpr int SRA_NW = 4;              // waves per block
constexpr int SRA_MAXA = 256;
constexpr int SRA_SPLIT_BLOCKS = 1024;  // the key-stationary pass splits the queries until it has about this many blocks (a constant: results do not depend on the device)
constexpr int SRA_MAX_SPLIT = 64;

struct SraGeo {
    int B, heads, d, A;
    long long N, M;
    float scale;
};

// 64 positions [p0, p0 + 64) of the d channels at `src` (rows `stride` apart) -> four tiles [DP][SRA_LS]; zero beyond `lim` and beyond d
template <int DP>
__device__ inline void sra_stage(float* dst, const float* __restrict__ src, int d, long long stride, long long p0, long long lim, int tid) {
#pragma unroll
    for (int e = tid; e < DP * 64; e += SRA_NW * 64) {
        const int pp = e & 63, c = e >> 6;
        const long long p = p0 + pp;
        dst[(pp >> 4) * DP * SRA_LS + c * SRA_LS + (pp & 15)] = (c < d && p < lim) ? src[(long long)c * stride + p] : 0.f;
    }
}

// one score tile: acc[p][n] = sum_c tile[c][p] st[c][n]
template <int KC>
__device__ inline f32x4 sra_score(const float* tile, const float (&st)[KC * 4], int g, int n) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(16 * t + 4 * g + u) * SRA_LS + n], st[t * 4 + u], acc, 0, 0, 0);
    return acc;
}

// acc[t][c][n] += sum_p tile[16 t + c][p] w[p][n]
template <int KC>
__device__ inline void sra_apply(const float* tile, const float (&w)[4], f32x4 (&acc)[KC], int g, int n) {
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (16 * t + n) * SRA_LS + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], w[r], acc[t], 0, 0, 0);
    }
}

// ---------------------------------------------------------------- forward: o, lse
template <int KC>
__global__ __launch_bounds__(SRA_NW * 64) void sra_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                              float* __restrict__ o, float* __restrict__ lse, SraGeo G) {
    constexpr int DP = KC * 16, TS = DP * SRA_LS;
    __shared__ __attribute__((aligned(16))) float sk[SRA_CH * TS];
    __shared__ __attribute__((aligned(16))) float sv[SRA_CH * TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z;
    const long long i = ((long long)blockIdx.x * SRA_NW + wave) * 16 + n;
    const bool qv = i < G.N;
    const long long ch0 = (long long)b * G.A + (long long)h * G.d;

    float qr[KC * 4];
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 16 * t + 4 * g + u;
            qr[t * 4 + u] = (qv && c < G.d) ? q[(ch0 + c) * G.N + i] : 0.f;
        }
    f32x4 oacc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lsum = 0.f;
    const float* kb = k + ch0 * G.M;
    const float* vb = v + ch0 * G.M;

    for (long long j0 = 0; j0 < G.M; j0 += 64) {
        __syncthreads();
        sra_stage<DP>(sk, kb, G.d, G.M, j0, G.M, tid);
        sra_stage<DP>(sv, vb, G.d, G.M, j0, G.M, tid);
        __syncthreads();
        const long long left = G.M - j0;
        const int nt = left >= 64 ? SRA_CH : (int)((left + 15) >> 4);
        float s[SRA_CH][4];
        float mx = -INFINITY;
#pragma unroll
        for (int ss = 0; ss < SRA_CH; ++ss) {
            if (ss < nt) {
                const f32x4 acc = sra_score<KC>(sk + ss * TS, qr, g, n);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[ss][r] = (ss * 16 + 4 * g + r < left) ? acc[r] * G.scale : -INFINITY;  // a key beyond M: weight exactly 0
                    mx = fmaxf(mx, s[ss][r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[ss][r] = -INFINITY;
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun, mx);   // finite from the first chunk on: key j0 is always inside M
        const float alpha = expf(mrun - mnew);
        mrun = mnew;
        lsum *= alpha;
#pragma unroll
        for (int t = 0; t < KC; ++t) oacc[t] *= alpha;
#pragma unroll
        for (int ss = 0; ss < SRA_CH; ++ss) {
            if (ss < nt) {
                float p[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = expf(s[ss][r] - mnew);
                    lsum += p[r];
                }
                sra_apply<KC>(sv + ss * TS, p, oacc, g, n);
            }
        }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (!qv) return;   // a query beyond N stores nothing
    const float inv = 1.f / lsum;
    if (g == 0) lse[((long long)b * G.heads + h) * G.N + i] = mrun + logf(lsum);
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * t + 4 * g + r;
            if (c < G.d) o[(ch0 + c) * G.N + i] = oacc[t][r] * inv;
        }
}

// ---------------------------------------------------------------- backward, query-stationary: D[b][h][i] = sum_c go o,  dq = scale dS^T k
template <int KC>
__global__ __launch_bounds__(SRA_NW * 64) void sra_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                const float* __restrict__ o, const float* __restrict__ lse, const float* __restrict__ go,
                                                                float* __restrict__ dq, float* __restrict__ dws, SraGeo G) {
    constexpr int DP = KC * 16, TS = DP * SRA_LS;
    __shared__ __attribute__((aligned(16))) float sk[SRA_CH * TS];
    __shared__ __attribute__((aligned(16))) float sv[SRA_CH * TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z;
    const long long i = ((long long)blockIdx.x * SRA_NW + wave) * 16 + n;
    const bool qv = i < G.N;
    const long long ch0 = (long long)b * G.A + (long long)h * G.d;
    const long long row = ((long long)b * G.heads + h) * G.N + i;

    float qr[KC * 4], gr[KC * 4];
    float dsum = 0.f;
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 16 * t + 4 * g + u;
            const bool ok = qv && c < G.d;
            const long long a = (ch0 + c) * G.N + i;
            qr[t * 4 + u] = ok ? q[a] : 0.f;
            gr[t * 4 + u] = ok ? go[a] : 0.f;
            if (ok) dsum += gr[t * 4 + u] * o[a];
        }
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    const float L = qv ? lse[row] : 0.f;
    if (qv && g == 0) dws[row] = dsum;
    f32x4 dacc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) dacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* kb = k + ch0 * G.M;
    const float* vb = v + ch0 * G.M;

    for (long long j0 = 0; j0 < G.M; j0 += 64) {
        __syncthreads();
        sra_stage<DP>(sk, kb, G.d, G.M, j0, G.M, tid);
        sra_stage<DP>(sv, vb, G.d, G.M, j0, G.M, tid);
        __syncthreads();
        const long long left = G.M - j0;
        const int nt = left >= 64 ? SRA_CH : (int)((left + 15) >> 4);
#pragma unroll
        for (int ss = 0; ss < SRA_CH; ++ss) {
            if (ss < nt) {
                const f32x4 sc = sra_score<KC>(sk + ss * TS, qr, g, n);
                const f32x4 dp = sra_score<KC>(sv + ss * TS, gr, g, n);
                float ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = (ss * 16 + 4 * g + r < left) ? expf(sc[r] * G.scale - L) : 0.f;
                    ds[r] = p * (dp[r] - dsum);
                }
                sra_apply<KC>(sk + ss * TS, ds, dacc, g, n);
            }
        }
    }
    if (!qv) return;
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * t + 4 * g + r;
            if (c < G.d) dq[(ch0 + c) * G.N + i] = dacc[t][r] * G.scale;
        }
}

// ---------------------------------------------------------------- backward, key-stationary: partial dk = scale q dS, dv = go P over one chunk of queries
// block = SRA_NW key tiles of one (sample, head) x one chunk of queries; q and go tiles of 64 queries are staged through LDS
template <int KC>
__global__ __launch_bounds__(SRA_NW * 64) void sra_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                 const float* __restrict__ lse, const float* __restrict__ dws, const float* __restrict__ go,
                                                                 float* __restrict__ dkp, float* __restrict__ dvp, long long qchunk, int JT, SraGeo G) {
    constexpr int DP = KC * 16, TS = DP * SRA_LS;
    __shared__ __attribute__((aligned(16))) float sq[SRA_CH * TS];
    __shared__ __attribute__((aligned(16))) float sg[SRA_CH * TS];
    __shared__ float sl[64], sd[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
    const int bh = blockIdx.z, b = bh / G.heads, h = bh - b * G.heads, split = blockIdx.y;
    const int jt = blockIdx.x * SRA_NW + wave;
    const long long j = (long long)jt * 16 + n;
    const bool kv = j < G.M;
    const long long ch0 = (long long)b * G.A + (long long)h * G.d;

    float kr[KC * 4], vr[KC * 4];
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 16 * t + 4 * g + u;
            const bool ok = kv && c < G.d;
            kr[t * 4 + u] = ok ? k[(ch0 + c) * G.M + j] : 0.f;
            vr[t * 4 + u] = ok ? v[(ch0 + c) * G.M + j] : 0.f;
        }
    f32x4 kacc[KC], vacc[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) {
        kacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        vacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const long long q0 = (long long)split * qchunk, q1 = q0 + qchunk < G.N ? q0 + qchunk : G.N;
    const float* qb = q + ch0 * G.N;
    const float* gb = go + ch0 * G.N;

    for (long long i0 = q0; i0 < q1; i0 += 64) {
        __syncthreads();
        sra_stage<DP>(sq, qb, G.d, G.N, i0, q1, tid);
        sra_stage<DP>(sg, gb, G.d, G.N, i0, q1, tid);
        if (tid < 64) {
            const long long ii = i0 + tid;
            sl[tid] = ii < q1 ? lse[(long long)bh * G.N + ii] : INFINITY;   // a query beyond the chunk: weight exactly 0
            sd[tid] = ii < q1 ? dws[(long long)bh * G.N + ii] : 0.f;
        }
        __syncthreads();
        const long long left = q1 - i0;
        const int nt = left >= 64 ? SRA_CH : (int)((left + 15) >> 4);
#pragma unroll
        for (int ss = 0; ss < SRA_CH; ++ss) {
            if (ss < nt) {
                const f32x4 sc = sra_score<KC>(sq + ss * TS, kr, g, n);   // [query 4 g + r][key n]
                const f32x4 dp = sra_score<KC>(sg + ss * TS, vr, g, n);
                float p[4], ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int iq = ss * 16 + 4 * g + r;
                    p[r] = kv ? expf(sc[r] * G.scale - sl[iq]) : 0.f;
                    ds[r] = p[r] * (dp[r] - sd[iq]);
                }
                sra_apply<KC>(sg + ss * TS, p, vacc, g, n);
                sra_apply<KC>(sq + ss * TS, ds, kacc, g, n);
            }
        }
    }
    if (jt >= JT) return;
    const long long mp = (long long)JT * 16;
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * t + 4 * g + r;
            if (c < G.d) {
                const long long a = (((long long)split * G.B + b) * G.A + (long long)h * G.d + c) * mp + j;
                dkp[a] = kacc[t][r] * G.scale;
                dvp[a] = vacc[t][r];
            }
        }
}

// dk, dv [B][A][M] = sum of the split partials, in split order
__global__ void sra_kv_sum_kernel(const float* __restrict__ dkp, const float* __restrict__ dvp, float* __restrict__ dk, float* __restrict__ dv, int nsplit,
                                  long long mp, long long rows, long long M) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * M) return;
    const long long jj = idx % M, rowi = idx / M;
    float sk = 0.f, sv = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const long long a = ((long long)s * rows + rowi) * mp + jj;
        sk += dkp[a];
        sv += dvp[a];
    }
    dk[idx] = sk;
    dv[idx] = sv;
}

// ---------------------------------------------------------------- host side
int check_args(const char* what, int b, int heads, int d, long long n, long long m, SraGeo& G) {
    MMIF_REQUIRE(d == 8 || d == 16 || d == 32, "%s: the head dimension must be 8, 16 or 32 (got %d)", what, d);
    MMIF_REQUIRE(heads >= 1 && (long long)heads * d <= SRA_MAXA, "%s: needs heads >= 1 and heads * d <= %d (got heads %d, d %d)", what, SRA_MAXA, heads, d);
    MMIF_REQUIRE(b >= 1 && (long long)b * heads <= 65535, "%s: needs 1 <= b and b * heads <= 65535 (got b %d, heads %d)", what, b, heads);
    MMIF_REQUIRE(n >= 1 && m >= 1 && n < (1ll << 30) && m < (1ll << 30), "%s: needs 1 <= n, m < 2^30 (got n %lld, m %lld)", what, n, m);
    MMIF_REQUIRE((long long)b * heads * d * (n > m ? n : m) / 256 < 0x7fffffffll, "%s: b * heads * d * max(n, m) too large (b %d, heads %d, d %d, n %lld, m %lld)", what, b, heads, d, n, m);
    G.B = b; G.heads = heads; G.d = d; G.A = heads * d; G.N = n; G.M = m; G.scale = 0.f;
    return MMIF_OK;
}

struct SraPlan {
    int JT, kgroups, nsplit;
    long long qchunk;
    size_t off_d, off_dkp, off_dvp, bytes;
};

SraPlan make_plan(const SraGeo& G) {
    SraPlan p;
    p.JT = (int)((G.M + 15) / 16);
    p.kgroups = (p.JT + SRA_NW - 1) / SRA_NW;
    const long long tiles = (G.N + 63) / 64, per = (long long)p.kgroups * G.B * G.heads;
    long long want = (SRA_SPLIT_BLOCKS + per - 1) / per;
    want = want < 1 ? 1 : (want > SRA_MAX_SPLIT ? SRA_MAX_SPLIT : want);
    if (want > tiles) want = tiles;
    p.qchunk = ((tiles + want - 1) / want) * 64;
    p.nsplit = (int)((G.N + p.qchunk - 1) / p.qchunk);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t part = up((size_t)p.nsplit * G.B * G.A * p.JT * 16 * sizeof(float));
    size_t o = 0;
    p.off_d = o;   o += up((size_t)G.B * G.heads * G.N * sizeof(float));
    p.off_dkp = o; o += part;
    p.off_dvp = o; o += part;
    p.bytes = o;
    return p;
}

#define SRA_DISPATCH(d, CALL)                             \
    if ((d) <= 16) { constexpr int KC = 1; CALL; }        \
    else { constexpr int KC = 2; CALL; }

}  // namespace
}  // namespace mmif

using namespace mmif;

extern "C" size_t mmif_sra_workspace(int32_t b, int32_t heads, int32_t d, int64_t n, int64_t m) {
    SraGeo G;
    if (check_args("mmif_sra_workspace", b, heads, d, n, m, G) != MMIF_OK) return 0;
    return make_plan(G).bytes;
}

extern "C" int mmif_sra_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int32_t b, int32_t heads, int32_t d, int64_t n, int64_t m,
                            float scale, void* stream) {
    SraGeo G;
    if (int rc = check_args("mmif_sra_fwd", b, heads, d, n, m, G)) return rc;
    MMIF_REQUIRE(q != nullptr && k != nullptr && v != nullptr && o != nullptr && lse != nullptr, "mmif_sra_fwd: null pointer");
    G.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(G.N, SRA_NW * 16), heads, b);
    SRA_DISPATCH(d, hipLaunchKernelGGL(sra_fwd_kernel<KC>, grid, dim3(SRA_NW * 64), 0, st, q, k, v, o, lse, G));
    return check_launch("sra fwd");
}

extern "C" int mmif_sra_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go, float* dq, float* dk, float* dv,
                            int32_t b, int32_t heads, int32_t d, int64_t n, int64_t m, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    SraGeo G;
    if (int rc = check_args("mmif_sra_bwd", b, heads, d, n, m, G)) return rc;
    MMIF_REQUIRE(q != nullptr && k != nullptr && v != nullptr && o != nullptr && lse != nullptr && go != nullptr && dq != nullptr && dk != nullptr &&
                     dv != nullptr && workspace != nullptr,
                 "mmif_sra_bwd: null pointer");
    G.scale = scale;
    const SraPlan p = make_plan(G);
    if (workspace_bytes < p.bytes) {
        set_error("mmif_sra_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* dws = (float*)(ws + p.off_d);
    float* dkp = (float*)(ws + p.off_dkp);
    float* dvp = (float*)(ws + p.off_dvp);
    const dim3 qgrid((unsigned)cdiv(G.N, SRA_NW * 16), heads, b);
    SRA_DISPATCH(d, hipLaunchKernelGGL(sra_bwd_q_kernel<KC>, qgrid, dim3(SRA_NW * 64), 0, st, q, k, v, o, lse, go, dq, dws, G));
    if (int rc = check_launch("sra bwd query pass")) return rc;
    const dim3 kgrid(p.kgroups, p.nsplit, b * heads);
    SRA_DISPATCH(d, hipLaunchKernelGGL(sra_bwd_kv_kernel<KC>, kgrid, dim3(SRA_NW * 64), 0, st, q, k, v, lse, dws, go, dkp, dvp, p.qchunk, p.JT, G));
    if (int rc = check_launch("sra bwd key pass")) return rc;
    const long long rows = (long long)b * G.A;
    hipLaunchKernelGGL(sra_kv_sum_kernel, dim3((unsigned)cdiv(rows * G.M, 256)), dim3(256), 0, st, dkp, dvp, dk, dv, p.nsplit, (long long)p.JT * 16, rows, G.M);
    return check_launch("sra bwd partial sum");
}
