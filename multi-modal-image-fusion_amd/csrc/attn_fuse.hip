// attention_fusion (reference core/fusion.py:42-81) for every tensor-level pooling mode, and SEDRFuse's strategy, on plain NCHW fp32:
//   s = spatial pool over channels [n][h*w]:  0 'sum', 1 'mean', 2 'l1', 3 'l2', 4 'linf' (max over channels),
//                                             5 sum_c softmax_c(|x|) |x| (SEDRFuse, reference core/model.py:271-281)
//   c = channel pool over the plane [n][c]:   0 'avg', 1 'max' (with the row-major position of the maximum, ci)
//   fs = wf(t1, t2, s1, s2),  fc = wf(t1, t2, c1, c2)  (weighted_fusion: fuse_join.hpp),  out = 'sa' fs | 'ca' fc | 'sca' (fs + fc) / 2 |
//   'wavg' wf(fs, fc, fs, fc) -- the arithmetic of mmif_fuse_join_* (include/mmif.h).
//
// A thread owns AF_PX = 4 consecutive pixels, a block a tile of 1024; the ownership is the same on the 16-byte path (h*w a multiple of 4 and
// every pointer 16-byte aligned) and on the scalar path, so both sum in the same order.
// pool        one block walks ALL channels of a (sample, tile): the spatial accumulators stay in registers, t1 and t2 are read once; per channel
//             every wave leaves one partial (sum, or maximum and position) of its 256 pixels in the workspace.
//             Where a sample has few tiles the channels are cut into chunks (AfGeo::K, a function of c and h*w alone), one block per (sample,
//             tile, chunk); the chunks' spatial accumulators go through the workspace and one small kernel folds them in chunk order.
// final       one wave per (sample, channel) finishes the partials in a fixed order; plane sums in double (fp32 only inside 256 pixels).
// join        element-wise over (sample, channel, tile): out.                                               forward: 5 planes of traffic
// bwd reduce  like pool: recomputes the join per element from the operands and the saved pools, sums the gradients with respect to s1, s2 over
//             the channels in registers and leaves per-wave partials of those with respect to c1, c2; for 'linf' it also finds the FIRST channel
//             holding the maximum, for mode 5 the log-sum-exp of |x|.
// bwd grad    element-wise: dt = direct terms + ds * ds/dx + dc * dc/dx.                                     backward: 8 planes
// Sub-gradients as torch's CPU autograd takes them: l1 sign(x) with sign(0) = 0; l2 x / |x|_2, 0 for a zero vector; linf all to the first channel
// holding the maximum; 'max' all to the first position in row-major order (max_pool2d; NOT amax's even split); mode 5 p_c (1 + |x_c| - s) sign(x_c).
// No atomics: every reduction order depends on (c, h, w) only, so results are bit-identical from run to run and a sample's results do not
// depend on the batch it sits in.  NaN inputs are out of scope (maxima and the clamp would not follow torch).
#include <float.h>
#include <limits.h>
#include <math.h>

#include <initializer_list>

#include "common.hpp"
#include "fuse_join.hpp"

namespace mmif {
namespace {

constexpr int AF_PX = 4;               // pixels per thread
constexpr int AF_TILE = 256 * AF_PX;   // pixels per block
constexpr int AF_POOL_BLOCKS = 1024;   // grid cap of the channel-walking kernels (grid-stride beyond; a constant: results do not depend on the device)
constexpr int AF_ELEM_BLOCKS = 4096;   // grid cap of the element-wise kernels
constexpr int AF_WAVES = 4;

constexpr int AF_ITEMS = 64;           // the channel-walking kernels cut the channels into chunks until a sample has about this many work items ...
constexpr int AF_MIN_CHUNK = 8;        // ... of at least this many channels each

struct AfGeo {
    int B, C, N, ntiles;
    int K, cpc;   // channel chunks of the channel-walking kernels and channels per chunk: functions of (c, h * w) only
};

template <bool VEC>
__device__ inline void af_ld4(const float* __restrict__ p, long long i, int nv, float (&v)[4]) {
    if (VEC) {   // nv is 0 or 4
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nv == 4) q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[i + j] : 0.f;
    }
}

template <bool VEC>
__device__ inline void af_ld4i(const int* __restrict__ p, long long i, int nv, int (&v)[4]) {
    if (VEC) {
        int4 q = make_int4(0, 0, 0, 0);
        if (nv == 4) q = *reinterpret_cast<const int4*>(p + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[i + j] : 0;
    }
}

template <bool VEC>
__device__ inline void af_st4(float* __restrict__ p, long long i, int nv, const float (&v)[4]) {
    if (VEC) {
        if (nv == 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[i + j] = v[j];
    }
}

template <bool VEC>
__device__ inline void af_st4i(int* __restrict__ p, long long i, int nv, const int (&v)[4]) {
    if (VEC) {
        if (nv == 4) *reinterpret_cast<int4*>(p + i) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) p[i + j] = v[j];
    }
}

__device__ inline float af_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline double af_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the larger value; among equals the smaller position (an empty slot is (-inf, INT_MAX))
__device__ inline void af_wave_max(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// ---------------------------------------------------------------- spatial pooling, one pixel
struct SpAcc {
    float a, m, d;   // a: the running sum / maximum; mode 5: a = sum exp(|x| - m) |x|, d = sum exp(|x| - m), m = the running maximum of |x|
};

template <int SM>
__device__ inline void sp_init(SpAcc& s) {
    s.a = SM == 4 ? -INFINITY : 0.f;
    s.m = 0.f;   // (|x| >= 0)
    s.d = 0.f;
}

template <int SM>
__device__ inline void sp_add(SpAcc& s, float x) {
    if (SM == 0 || SM == 1) s.a += x;
    else if (SM == 2) s.a += fabsf(x);
    else if (SM == 3) s.a += x * x;
    else if (SM == 4) s.a = x > s.a ? x : s.a;
    else {
        const float v = fabsf(x);
        if (v > s.m) {
            const float sc = expf(s.m - v);
            s.d = s.d * sc + 1.f;
            s.a = s.a * sc + v;
            s.m = v;
        } else {
            const float e = expf(v - s.m);
            s.d += e;
            s.a += e * v;
        }
    }
}

template <int SM>
__device__ inline float sp_finish(const SpAcc& s, int c) {
    if (SM == 1) return s.a / (float)c;
    if (SM == 3) return sqrtf(s.a);
    if (SM == 5) return s.a / s.d;
    return s.a;
}

// ds/dx of one element times the upstream ds; aux: 'linf' the first channel holding the maximum, mode 5 the log-sum-exp of |x| (as bits)
template <int SM>
__device__ inline float sp_grad(float x, float s, float ds, int aux, int ch, int c) {
    if (SM == 0) return ds;
    if (SM == 1) return ds / (float)c;
    if (SM == 2) return x > 0.f ? ds : (x < 0.f ? -ds : 0.f);
    if (SM == 3) return s > 0.f ? x * (ds / s) : 0.f;
    if (SM == 4) return aux == ch ? ds : 0.f;
    const float v = fabsf(x);
    const float p = expf(v - __int_as_float(aux));
    const float d = ds * (p * (1.f + v - s));
    return x > 0.f ? d : (x < 0.f ? -d : 0.f);
}

// ---------------------------------------------------------------- the join, one element
template <int MODE>
__device__ inline float af_join(float a, float b, float s1, float s2, float c1, float c2) {
    float fs = 0.f, fc = 0.f;
    if (MODE != 1) fs = wf_fwd(a, b, s1, s2).f;
    if (MODE != 0) fc = wf_fwd(a, b, c1, c2).f;
    if (MODE == 0) return fs;
    if (MODE == 1) return fc;
    if (MODE == 2) return (fs + fc) / 2.0f;
    return wf_fwd(fs, fc, fs, fc).f;
}

struct AfGrad {
    float d1, d2;      // direct terms of dt1, dt2
    float das, dbs;    // with respect to s1, s2 of this pixel
    float dac, dbc;    // with respect to c1, c2 of this channel
};

template <int MODE>
__device__ inline AfGrad af_join_bwd(float a, float b, float gi, float s1, float s2, float c1, float c2) {
    AfGrad o{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Wf ws{}, wc{};
    if (MODE != 1) ws = wf_fwd(a, b, s1, s2);
    if (MODE != 0) wc = wf_fwd(a, b, c1, c2);
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
    if (MODE != 1) {
        wf_bwd(ws, a, b, dfs, o.das, o.dbs);
        o.d1 += dfs * ws.w;
        o.d2 += dfs * (1.f - ws.w);
    }
    if (MODE != 0) {
        wf_bwd(wc, a, b, dfc, o.dac, o.dbc);
        o.d1 += dfc * wc.w;
        o.d2 += dfc * (1.f - wc.w);
    }
    return o;
}

__device__ inline size_t af_part_index(const AfGeo& q, long long row, int tile, int wave) {
    return ((size_t)row * q.ntiles + tile) * AF_WAVES + wave;
}

// ---------------------------------------------------------------- forward: both pools in one read of t1, t2.  SM / CM -1: that pool is not wanted
template <int SM, int CM, bool VEC>
__global__ __launch_bounds__(256) void af_pool_kernel(const float* __restrict__ t1, const float* __restrict__ t2, float* __restrict__ s1,
                                                      float* __restrict__ s2, float* __restrict__ pa, float* __restrict__ pb, int* __restrict__ ia,
                                                      int* __restrict__ ib, float* __restrict__ spart, AfGeo q) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long items = (long long)q.B * q.ntiles * q.K;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int k = (int)(it % q.K);
        const int tile = (int)((it / q.K) % q.ntiles);
        const long long b = it / ((long long)q.K * q.ntiles);
        const int p0 = tile * AF_TILE + tid * AF_PX;
        const int nv = min(AF_PX, max(0, q.N - p0));
        SpAcc a1[AF_PX], a2[AF_PX];
#pragma unroll
        for (int j = 0; j < AF_PX; ++j) { sp_init<SM>(a1[j]); sp_init<SM>(a2[j]); }
        const int ch1 = min(q.C, (k + 1) * q.cpc);
        for (int ch = k * q.cpc; ch < ch1; ++ch) {
            const long long row = b * q.C + ch;
            float x1[AF_PX], x2[AF_PX];
            af_ld4<VEC>(t1, row * q.N + p0, nv, x1);
            af_ld4<VEC>(t2, row * q.N + p0, nv, x2);
            if (SM >= 0) {
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) { sp_add<SM>(a1[j], x1[j]); sp_add<SM>(a2[j], x2[j]); }
            }
            if (CM == 0) {   // (pixels past the plane were loaded as 0)
                const float u1 = af_wave_sum(((x1[0] + x1[1]) + x1[2]) + x1[3]);
                const float u2 = af_wave_sum(((x2[0] + x2[1]) + x2[2]) + x2[3]);
                if (lane == 0) {
                    const size_t k = af_part_index(q, row, tile, wave);
                    pa[k] = u1;
                    pb[k] = u2;
                }
            }
            if (CM == 1) {
                float v1 = -INFINITY, v2 = -INFINITY;
                int i1 = INT_MAX, i2 = INT_MAX;
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) {
                    if (j < nv && x1[j] > v1) { v1 = x1[j]; i1 = p0 + j; }
                    if (j < nv && x2[j] > v2) { v2 = x2[j]; i2 = p0 + j; }
                }
                af_wave_max(v1, i1);
                af_wave_max(v2, i2);
                if (lane == 0) {
                    const size_t k = af_part_index(q, row, tile, wave);
                    pa[k] = v1; ia[k] = i1;
                    pb[k] = v2; ib[k] = i2;
                }
            }
        }
        if (SM >= 0 && q.K == 1) {
            float o1[AF_PX], o2[AF_PX];
#pragma unroll
            for (int j = 0; j < AF_PX; ++j) { o1[j] = sp_finish<SM>(a1[j], q.C); o2[j] = sp_finish<SM>(a2[j], q.C); }
            af_st4<VEC>(s1, b * q.N + p0, nv, o1);
            af_st4<VEC>(s2, b * q.N + p0, nv, o2);
        }
        if (SM >= 0 && q.K > 1) {   // the chunk's raw accumulators: af_sp_combine_kernel folds the chunks in order
            const long long arr = (long long)q.K * q.B * q.N, at = ((long long)k * q.B + b) * q.N + p0;
            float o1[AF_PX], o2[AF_PX];
#pragma unroll
            for (int j = 0; j < AF_PX; ++j) { o1[j] = a1[j].a; o2[j] = a2[j].a; }
            af_st4<VEC>(spart, at, nv, o1);
            af_st4<VEC>(spart, arr + at, nv, o2);
            if (SM == 5) {
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) { o1[j] = a1[j].m; o2[j] = a2[j].m; }
                af_st4<VEC>(spart, 2 * arr + at, nv, o1);
                af_st4<VEC>(spart, 3 * arr + at, nv, o2);
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) { o1[j] = a1[j].d; o2[j] = a2[j].d; }
                af_st4<VEC>(spart, 4 * arr + at, nv, o1);
                af_st4<VEC>(spart, 5 * arr + at, nv, o2);
            }
        }
    }
}

// fold of two partial accumulators of one pixel, the earlier chunk first
template <int SM>
__device__ inline void sp_merge(SpAcc& s, const SpAcc& o) {
    if (SM == 4) s.a = o.a > s.a ? o.a : s.a;
    else if (SM == 5) {
        const float m = o.m > s.m ? o.m : s.m;
        const float e0 = expf(s.m - m), e1 = expf(o.m - m);
        s.d = s.d * e0 + o.d * e1;
        s.a = s.a * e0 + o.a * e1;
        s.m = m;
    } else s.a += o.a;
}

// the spatial pools of a chunked pooling pass: per pixel, the chunks in order
template <int SM>
__global__ __launch_bounds__(256) void af_sp_combine_kernel(const float* __restrict__ spart, float* __restrict__ s1, float* __restrict__ s2, AfGeo q) {
    const long long total = (long long)q.B * q.N, arr = total * q.K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            SpAcc acc;
            for (int k = 0; k < q.K; ++k) {
                const long long at = (long long)k * total + i;
                SpAcc o{spart[t * arr + at], 0.f, 0.f};
                if (SM == 5) { o.m = spart[(2 + t) * arr + at]; o.d = spart[(4 + t) * arr + at]; }
                if (k == 0) acc = o;
                else sp_merge<SM>(acc, o);
            }
            (t == 0 ? s1 : s2)[i] = sp_finish<SM>(acc, q.C);
        }
    }
}

// second stage of a plane sum: one wave per (sample, channel), the partials in a fixed order, in double; MEAN: divided by the plane size
template <bool MEAN>
__global__ __launch_bounds__(256) void af_sum_final_kernel(const float* __restrict__ pa, const float* __restrict__ pb, float* __restrict__ o1,
                                                           float* __restrict__ o2, AfGeo q) {
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)q.B * q.C;
    const long long np = (long long)q.ntiles * AF_WAVES;
    for (long long row = (long long)blockIdx.x * AF_WAVES + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * AF_WAVES) {
        double a = 0.0, b = 0.0;
        for (long long k = lane; k < np; k += 64) {
            a += (double)pa[row * np + k];
            b += (double)pb[row * np + k];
        }
        a = af_wave_sum(a);
        b = af_wave_sum(b);
        if (lane == 0) {
            o1[row] = (float)(MEAN ? a / (double)q.N : a);
            o2[row] = (float)(MEAN ? b / (double)q.N : b);
        }
    }
}

// second stage of a plane maximum: the first position in row-major order among equals
__global__ __launch_bounds__(256) void af_max_final_kernel(const float* __restrict__ pa, const float* __restrict__ pb, const int* __restrict__ ia,
                                                           const int* __restrict__ ib, float* __restrict__ c1, float* __restrict__ c2,
                                                           int* __restrict__ ci1, int* __restrict__ ci2, AfGeo q) {
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)q.B * q.C;
    const long long np = (long long)q.ntiles * AF_WAVES;
    for (long long row = (long long)blockIdx.x * AF_WAVES + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * AF_WAVES) {
        float v1 = -INFINITY, v2 = -INFINITY;
        int i1 = INT_MAX, i2 = INT_MAX;
        for (long long k = lane; k < np; k += 64) {
            const float u1 = pa[row * np + k], u2 = pb[row * np + k];
            const int j1 = ia[row * np + k], j2 = ib[row * np + k];
            if (u1 > v1 || (u1 == v1 && j1 < i1)) { v1 = u1; i1 = j1; }
            if (u2 > v2 || (u2 == v2 && j2 < i2)) { v2 = u2; i2 = j2; }
        }
        af_wave_max(v1, i1);
        af_wave_max(v2, i2);
        if (lane == 0) {
            c1[row] = v1; ci1[row] = i1;
            c2[row] = v2; ci2[row] = i2;
        }
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void af_join_kernel(const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ s1,
                                                      const float* __restrict__ s2, const float* __restrict__ c1, const float* __restrict__ c2,
                                                      float* __restrict__ out, AfGeo q) {
    const long long items = (long long)q.B * q.C * q.ntiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int tile = (int)(it % q.ntiles);
        const long long row = it / q.ntiles, b = row / q.C;
        const int p0 = tile * AF_TILE + (int)threadIdx.x * AF_PX;
        const int nv = min(AF_PX, max(0, q.N - p0));
        if (nv == 0) continue;
        float x1[AF_PX], x2[AF_PX], sa[AF_PX] = {0.f, 0.f, 0.f, 0.f}, sb[AF_PX] = {0.f, 0.f, 0.f, 0.f}, o[AF_PX];
        af_ld4<VEC>(t1, row * q.N + p0, nv, x1);
        af_ld4<VEC>(t2, row * q.N + p0, nv, x2);
        if (MODE != 1) {
            af_ld4<VEC>(s1, b * q.N + p0, nv, sa);
            af_ld4<VEC>(s2, b * q.N + p0, nv, sb);
        }
        float ca = 0.f, cb = 0.f;
        if (MODE != 0) { ca = c1[row]; cb = c2[row]; }
#pragma unroll
        for (int j = 0; j < AF_PX; ++j) o[j] = af_join<MODE>(x1[j], x2[j], sa[j], sb[j], ca, cb);
        af_st4<VEC>(out, row * q.N + p0, nv, o);
    }
}

// ---------------------------------------------------------------- backward, first pass.  AUX 4: find the first channel holding the 'linf' maximum
// (int words in aux); AUX 5: the log-sum-exp of |x| over the channels (float words in aux); 0: neither
template <int MODE, int AUX, bool VEC>
__global__ __launch_bounds__(256) void af_bwd_reduce_kernel(const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ g,
                                                            const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ c1,
                                                            const float* __restrict__ c2, float* __restrict__ ds1, float* __restrict__ ds2,
                                                            int* __restrict__ aux1, int* __restrict__ aux2, float* __restrict__ pa,
                                                            float* __restrict__ pb, float* __restrict__ spart, AfGeo q) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long items = (long long)q.B * q.ntiles * q.K;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int k = (int)(it % q.K);
        const int tile = (int)((it / q.K) % q.ntiles);
        const long long b = it / ((long long)q.K * q.ntiles);
        const int p0 = tile * AF_TILE + tid * AF_PX;
        const int nv = min(AF_PX, max(0, q.N - p0));
        float sa[AF_PX] = {0.f, 0.f, 0.f, 0.f}, sb[AF_PX] = {0.f, 0.f, 0.f, 0.f};
        if (MODE != 1) {
            af_ld4<VEC>(s1, b * q.N + p0, nv, sa);
            af_ld4<VEC>(s2, b * q.N + p0, nv, sb);
        }
        float da[AF_PX] = {0.f, 0.f, 0.f, 0.f}, db[AF_PX] = {0.f, 0.f, 0.f, 0.f};
        int k1[AF_PX] = {-1, -1, -1, -1}, k2[AF_PX] = {-1, -1, -1, -1};
        SpAcc l1[AF_PX], l2[AF_PX];
#pragma unroll
        for (int j = 0; j < AF_PX; ++j) { sp_init<5>(l1[j]); sp_init<5>(l2[j]); }
        const int ch1 = min(q.C, (k + 1) * q.cpc);
        for (int ch = k * q.cpc; ch < ch1; ++ch) {
            const long long row = b * q.C + ch;
            float x1[AF_PX], x2[AF_PX], gg[AF_PX];
            af_ld4<VEC>(t1, row * q.N + p0, nv, x1);
            af_ld4<VEC>(t2, row * q.N + p0, nv, x2);
            af_ld4<VEC>(g, row * q.N + p0, nv, gg);
            float ca = 0.f, cb = 0.f;
            if (MODE != 0) { ca = c1[row]; cb = c2[row]; }
            float wa = 0.f, wb = 0.f;
#pragma unroll
            for (int j = 0; j < AF_PX; ++j) {
                if (j < nv) {
                    const AfGrad e = af_join_bwd<MODE>(x1[j], x2[j], gg[j], sa[j], sb[j], ca, cb);
                    da[j] += e.das;
                    db[j] += e.dbs;
                    wa += e.dac;
                    wb += e.dbc;
                    if (AUX == 4) {
                        if (k1[j] < 0 && x1[j] == sa[j]) k1[j] = ch;
                        if (k2[j] < 0 && x2[j] == sb[j]) k2[j] = ch;
                    }
                    if (AUX == 5) { sp_add<5>(l1[j], x1[j]); sp_add<5>(l2[j], x2[j]); }
                }
            }
            if (MODE != 0) {
                wa = af_wave_sum(wa);
                wb = af_wave_sum(wb);
                if (lane == 0) {
                    const size_t k = af_part_index(q, row, tile, wave);
                    pa[k] = wa;
                    pb[k] = wb;
                }
            }
        }
        if (MODE != 1 && q.K > 1) {   // the chunk's raw sums: af_ds_combine_kernel folds the chunks in order
            const long long arr = (long long)q.K * q.B * q.N, at = ((long long)k * q.B + b) * q.N + p0;
            af_st4<VEC>(spart, at, nv, da);
            af_st4<VEC>(spart, arr + at, nv, db);
            if (AUX == 4) {
                af_st4i<VEC>((int*)spart, 2 * arr + at, nv, k1);
                af_st4i<VEC>((int*)spart, 3 * arr + at, nv, k2);
            }
            if (AUX == 5) {
                float o1[AF_PX], o2[AF_PX];
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) { o1[j] = l1[j].m; o2[j] = l2[j].m; }
                af_st4<VEC>(spart, 2 * arr + at, nv, o1);
                af_st4<VEC>(spart, 3 * arr + at, nv, o2);
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) { o1[j] = l1[j].d; o2[j] = l2[j].d; }
                af_st4<VEC>(spart, 4 * arr + at, nv, o1);
                af_st4<VEC>(spart, 5 * arr + at, nv, o2);
            }
        }
        if (MODE != 1 && q.K == 1) {
            af_st4<VEC>(ds1, b * q.N + p0, nv, da);
            af_st4<VEC>(ds2, b * q.N + p0, nv, db);
            if (AUX == 5) {
#pragma unroll
                for (int j = 0; j < AF_PX; ++j) {
                    k1[j] = __float_as_int(l1[j].m + logf(l1[j].d));
                    k2[j] = __float_as_int(l2[j].m + logf(l2[j].d));
                }
            }
            if (AUX != 0) {
                af_st4i<VEC>(aux1, b * q.N + p0, nv, k1);
                af_st4i<VEC>(aux2, b * q.N + p0, nv, k2);
            }
        }
    }
}

// ds1, ds2 (and what 'linf' / mode 5 need) of a chunked reduction pass: per pixel, the chunks in order
template <int AUX>
__global__ __launch_bounds__(256) void af_ds_combine_kernel(const float* __restrict__ spart, float* __restrict__ ds1, float* __restrict__ ds2,
                                                            int* __restrict__ aux1, int* __restrict__ aux2, AfGeo q) {
    const long long total = (long long)q.B * q.N, arr = total * q.K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float d = 0.f;
            int first = -1;
            SpAcc l;
            for (int k = 0; k < q.K; ++k) {
                const long long at = (long long)k * total + i;
                const float v = spart[t * arr + at];
                d = k == 0 ? v : d + v;
                if (AUX == 4) {
                    const int c = ((const int*)spart)[(2 + t) * arr + at];
                    if (first < 0) first = c;
                }
                if (AUX == 5) {
                    const SpAcc o{0.f, spart[(2 + t) * arr + at], spart[(4 + t) * arr + at]};
                    if (k == 0) l = o;
                    else sp_merge<5>(l, o);
                }
            }
            (t == 0 ? ds1 : ds2)[i] = d;
            if (AUX == 4) (t == 0 ? aux1 : aux2)[i] = first;
            if (AUX == 5) (t == 0 ? aux1 : aux2)[i] = __float_as_int(l.m + logf(l.d));
        }
    }
}

// ---------------------------------------------------------------- backward, second pass.  SM / CM -1: the mode has no such pool
template <int MODE, int SM, int CM, bool VEC>
__global__ __launch_bounds__(256) void af_bwd_grad_kernel(const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ g,
                                                          const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ c1,
                                                          const float* __restrict__ c2, const int* __restrict__ ci1, const int* __restrict__ ci2,
                                                          const float* __restrict__ ds1, const float* __restrict__ ds2, const int* __restrict__ aux1,
                                                          const int* __restrict__ aux2, const float* __restrict__ dc1, const float* __restrict__ dc2,
                                                          float* __restrict__ dt1, float* __restrict__ dt2, AfGeo q) {
    const long long items = (long long)q.B * q.C * q.ntiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int tile = (int)(it % q.ntiles);
        const long long row = it / q.ntiles, b = row / q.C;
        const int ch = (int)(row - b * q.C);
        const int p0 = tile * AF_TILE + (int)threadIdx.x * AF_PX;
        const int nv = min(AF_PX, max(0, q.N - p0));
        if (nv == 0) continue;
        float x1[AF_PX], x2[AF_PX], gg[AF_PX];
        float sa[AF_PX] = {0.f, 0.f, 0.f, 0.f}, sb[AF_PX] = {0.f, 0.f, 0.f, 0.f}, da[AF_PX] = {0.f, 0.f, 0.f, 0.f}, db[AF_PX] = {0.f, 0.f, 0.f, 0.f};
        int k1[AF_PX] = {0, 0, 0, 0}, k2[AF_PX] = {0, 0, 0, 0};
        af_ld4<VEC>(t1, row * q.N + p0, nv, x1);
        af_ld4<VEC>(t2, row * q.N + p0, nv, x2);
        af_ld4<VEC>(g, row * q.N + p0, nv, gg);
        if (SM >= 0) {
            af_ld4<VEC>(s1, b * q.N + p0, nv, sa);
            af_ld4<VEC>(s2, b * q.N + p0, nv, sb);
            af_ld4<VEC>(ds1, b * q.N + p0, nv, da);
            af_ld4<VEC>(ds2, b * q.N + p0, nv, db);
            if (SM == 4 || SM == 5) {
                af_ld4i<VEC>(aux1, b * q.N + p0, nv, k1);
                af_ld4i<VEC>(aux2, b * q.N + p0, nv, k2);
            }
        }
        float ca = 0.f, cb = 0.f, dca = 0.f, dcb = 0.f;
        int pi1 = -1, pi2 = -1;
        if (CM >= 0) {
            ca = c1[row]; cb = c2[row];
            dca = dc1[row]; dcb = dc2[row];
            if (CM == 0) { dca = dca / (float)q.N; dcb = dcb / (float)q.N; }
            if (CM == 1) { pi1 = ci1[row]; pi2 = ci2[row]; }
        }
        float o1[AF_PX], o2[AF_PX];
#pragma unroll
        for (int j = 0; j < AF_PX; ++j) {
            const AfGrad e = af_join_bwd<MODE>(x1[j], x2[j], gg[j], sa[j], sb[j], ca, cb);
            float d1 = e.d1, d2 = e.d2;
            if (SM >= 0) {
                d1 += sp_grad<SM>(x1[j], sa[j], da[j], k1[j], ch, q.C);
                d2 += sp_grad<SM>(x2[j], sb[j], db[j], k2[j], ch, q.C);
            }
            if (CM == 0) { d1 += dca; d2 += dcb; }
            if (CM == 1) {
                if (p0 + j == pi1) d1 += dca;
                if (p0 + j == pi2) d2 += dcb;
            }
            o1[j] = d1;
            o2[j] = d2;
        }
        af_st4<VEC>(dt1, row * q.N + p0, nv, o1);
        af_st4<VEC>(dt2, row * q.N + p0, nv, o2);
    }
}

// ---------------------------------------------------------------- host side
struct AfPlan {
    bool sp, ch, cmax, aux;
    size_t off_pa, off_pb, off_ia, off_ib, off_ds1, off_ds2, off_aux1, off_aux2, off_dc1, off_dc2, off_spart, bytes;
};

int af_check(const char* what, int n, int c, int h, int w, int mode, int sm, int cm, AfGeo& q, AfPlan& p) {
    MMIF_REQUIRE(n >= 1 && n <= 65535 && c >= 1 && c <= 65535 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 30),
                 "%s: needs 1 <= n <= 65535, 1 <= c <= 65535, h, w >= 1 and h * w < 2^30 (got n %d, c %d, h %d, w %d)", what, n, c, h, w);
    MMIF_REQUIRE(mode >= 0 && mode <= 3, "%s: mode %d (0 'sa', 1 'ca', 2 'sca', 3 'wavg')", what, mode);
    MMIF_REQUIRE(sm >= 0 && sm <= 5, "%s: spatial mode %d (0 'sum', 1 'mean', 2 'l1', 3 'l2', 4 'linf', 5 softmax-weighted l1)", what, sm);
    MMIF_REQUIRE(cm >= 0 && cm <= 1, "%s: channel mode %d (0 'avg', 1 'max')", what, cm);
    q.B = n; q.C = c; q.N = h * w;
    q.ntiles = (q.N + AF_TILE - 1) / AF_TILE;
    int want = (AF_ITEMS + q.ntiles - 1) / q.ntiles;
    const int most = (c + AF_MIN_CHUNK - 1) / AF_MIN_CHUNK;
    want = want < most ? want : most;
    q.cpc = (c + want - 1) / want;
    q.K = (c + q.cpc - 1) / q.cpc;
    p.sp = mode != 1;
    p.ch = mode != 0;
    p.cmax = p.ch && cm == 1;
    p.aux = p.sp && (sm == 4 || sm == 5);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t parts = p.ch ? up((size_t)n * c * q.ntiles * AF_WAVES * 4) : 0;
    const size_t pix = p.sp ? up((size_t)n * q.N * 4) : 0;
    const size_t rows = p.ch ? up((size_t)n * c * 4) : 0;
    size_t o = 0;
    p.off_pa = o;   o += parts;
    p.off_pb = o;   o += parts;
    p.off_ia = o;   o += p.cmax ? parts : 0;
    p.off_ib = o;   o += p.cmax ? parts : 0;
    p.off_ds1 = o;  o += pix;
    p.off_ds2 = o;  o += pix;
    p.off_aux1 = o; o += p.aux ? pix : 0;
    p.off_aux2 = o; o += p.aux ? pix : 0;
    p.off_dc1 = o;  o += rows;
    p.off_dc2 = o;  o += rows;
    p.off_spart = o; o += (p.sp && q.K > 1) ? up((size_t)6 * q.K * n * q.N * 4) : 0;   // up to six arrays [K][n][h*w]
    p.bytes = o;
    return MMIF_OK;
}

int af_check_pools(const char* what, const AfPlan& p, const void* s1, const void* s2, const void* c1, const void* c2, const void* ci1,
                   const void* ci2) {
    MMIF_REQUIRE((s1 != nullptr) == p.sp && (s2 != nullptr) == p.sp, "%s: the mode %s the spatial pools", what, p.sp ? "needs" : "takes no");
    MMIF_REQUIRE((c1 != nullptr) == p.ch && (c2 != nullptr) == p.ch, "%s: the mode %s the channel pools", what, p.ch ? "needs" : "takes no");
    MMIF_REQUIRE((ci1 != nullptr) == p.cmax && (ci2 != nullptr) == p.cmax, "%s: the positions go with channel mode 'max' only, and are %s here", what,
                 p.cmax ? "needed" : "not taken");
    return MMIF_OK;
}

bool af_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (((uintptr_t)p & 15) != 0) return false;   // (NULL counts as aligned)
    return true;
}

unsigned af_grid(long long items, int cap) { return (unsigned)(items < cap ? items : cap); }

#define AF_SWITCH_SM(sm, CALL)                                 \
    switch (sm) {                                              \
        case -1: { constexpr int SM = -1; CALL; } break;       \
        case 0: { constexpr int SM = 0; CALL; } break;         \
        case 1: { constexpr int SM = 1; CALL; } break;         \
        case 2: { constexpr int SM = 2; CALL; } break;         \
        case 3: { constexpr int SM = 3; CALL; } break;         \
        case 4: { constexpr int SM = 4; CALL; } break;         \
        default: { constexpr int SM = 5; CALL; } break;        \
    }
#define AF_SWITCH_CM(cm, CALL)                                 \
    switch (cm) {                                              \
        case -1: { constexpr int CM = -1; CALL; } break;       \
        case 0: { constexpr int CM = 0; CALL; } break;         \
        default: { constexpr int CM = 1; CALL; } break;        \
    }
#define AF_SWITCH_MODE(mode, CALL)                             \
    switch (mode) {                                            \
        case 0: { constexpr int MODE = 0; CALL; } break;       \
        case 1: { constexpr int MODE = 1; CALL; } break;       \
        case 2: { constexpr int MODE = 2; CALL; } break;       \
        default: { constexpr int MODE = 3; CALL; } break;      \
    }

template <int SM, int CM>
void launch_pool(bool vec, dim3 grid, dim3 gpix, hipStream_t st, const float* t1, const float* t2, float* s1, float* s2, float* pa, float* pb, int* ia,
                 int* ib, float* spart, const AfGeo& q) {
    if constexpr (SM >= 0 || CM >= 0) {
        if (vec) hipLaunchKernelGGL((af_pool_kernel<SM, CM, true>), grid, dim3(256), 0, st, t1, t2, s1, s2, pa, pb, ia, ib, spart, q);
        else hipLaunchKernelGGL((af_pool_kernel<SM, CM, false>), grid, dim3(256), 0, st, t1, t2, s1, s2, pa, pb, ia, ib, spart, q);
    }
    if constexpr (SM >= 0) {
        if (q.K > 1) hipLaunchKernelGGL(af_sp_combine_kernel<SM>, gpix, dim3(256), 0, st, spart, s1, s2, q);
    }
}

template <int MODE>
void launch_join(bool vec, dim3 grid, hipStream_t st, const float* t1, const float* t2, const float* s1, const float* s2, const float* c1,
                 const float* c2, float* out, const AfGeo& q) {
    if (vec) hipLaunchKernelGGL((af_join_kernel<MODE, true>), grid, dim3(256), 0, st, t1, t2, s1, s2, c1, c2, out, q);
    else hipLaunchKernelGGL((af_join_kernel<MODE, false>), grid, dim3(256), 0, st, t1, t2, s1, s2, c1, c2, out, q);
}

template <int MODE, int AUX>
void launch_reduce(bool vec, dim3 grid, hipStream_t st, const float* t1, const float* t2, const float* g, const float* s1, const float* s2,
                   const float* c1, const float* c2, float* ds1, float* ds2, int* aux1, int* aux2, float* pa, float* pb, float* spart, dim3 gpix,
                   const AfGeo& q) {
    if constexpr (MODE != 1 || AUX == 0) {
        if (vec)
            hipLaunchKernelGGL((af_bwd_reduce_kernel<MODE, AUX, true>), grid, dim3(256), 0, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, q);
        else
            hipLaunchKernelGGL((af_bwd_reduce_kernel<MODE, AUX, false>), grid, dim3(256), 0, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, q);
        if (MODE != 1 && q.K > 1) hipLaunchKernelGGL(af_ds_combine_kernel<AUX>, gpix, dim3(256), 0, st, spart, ds1, ds2, aux1, aux2, q);
    }
}

template <int MODE>
void launch_reduce_aux(int aux, bool vec, dim3 grid, hipStream_t st, const float* t1, const float* t2, const float* g, const float* s1, const float* s2,
                       const float* c1, const float* c2, float* ds1, float* ds2, int* aux1, int* aux2, float* pa, float* pb, float* spart, dim3 gpix,
                       const AfGeo& q) {
    if (aux == 4) launch_reduce<MODE, 4>(vec, grid, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, gpix, q);
    else if (aux == 5) launch_reduce<MODE, 5>(vec, grid, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, gpix, q);
    else launch_reduce<MODE, 0>(vec, grid, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, gpix, q);
}

template <int MODE, int SM, int CM>
void launch_grad(bool vec, dim3 grid, hipStream_t st, const float* t1, const float* t2, const float* g, const float* s1, const float* s2,
                 const float* c1, const float* c2, const int* ci1, const int* ci2, const float* ds1, const float* ds2, const int* aux1, const int* aux2,
                 const float* dc1, const float* dc2, float* dt1, float* dt2, const AfGeo& q) {
    if constexpr ((MODE != 1) == (SM >= 0) && (MODE != 0) == (CM >= 0)) {
        if (vec)
            hipLaunchKernelGGL((af_bwd_grad_kernel<MODE, SM, CM, true>), grid, dim3(256), 0, st, t1, t2, g, s1, s2, c1, c2, ci1, ci2, ds1, ds2, aux1, aux2,
                               dc1, dc2, dt1, dt2, q);
        else
            hipLaunchKernelGGL((af_bwd_grad_kernel<MODE, SM, CM, false>), grid, dim3(256), 0, st, t1, t2, g, s1, s2, c1, c2, ci1, ci2, ds1, ds2, aux1, aux2,
                               dc1, dc2, dt1, dt2, q);
    }
}

}  // namespace
}  // namespace mmif

using namespace mmif;

extern "C" size_t mmif_attn_fuse_workspace(int32_t n, int32_t c, int32_t h, int32_t w, int32_t mode, int32_t spatial_mode, int32_t channel_mode) {
    AfGeo q;
    AfPlan p;
    if (af_check("mmif_attn_fuse_workspace", n, c, h, w, mode, spatial_mode, channel_mode, q, p) != MMIF_OK) return 0;
    return p.bytes;
}

extern "C" int mmif_attn_fuse_fwd(const float* t1, const float* t2, float* out, float* s1, float* s2, float* c1, float* c2, int32_t* ci1, int32_t* ci2,
                                  int32_t n, int32_t c, int32_t h, int32_t w, int32_t mode, int32_t spatial_mode, int32_t channel_mode, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    AfGeo q;
    AfPlan p;
    if (int rc = af_check("mmif_attn_fuse_fwd", n, c, h, w, mode, spatial_mode, channel_mode, q, p)) return rc;
    MMIF_REQUIRE(t1 != nullptr && t2 != nullptr && out != nullptr && workspace != nullptr, "mmif_attn_fuse_fwd: null pointer");
    if (int rc = af_check_pools("mmif_attn_fuse_fwd", p, s1, s2, c1, c2, ci1, ci2)) return rc;
    if (workspace_bytes < p.bytes) {
        set_error("mmif_attn_fuse_fwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pa = (float*)(ws + p.off_pa);
    float* pb = (float*)(ws + p.off_pb);
    int* ia = (int*)(ws + p.off_ia);
    int* ib = (int*)(ws + p.off_ib);
    float* spart = (float*)(ws + p.off_spart);
    const bool vec = q.N % 4 == 0 && af_aligned({t1, t2, out, s1, s2, workspace});
    const int sm = p.sp ? spatial_mode : -1, cm = p.ch ? channel_mode : -1;
    const dim3 gpool(af_grid((long long)q.B * q.ntiles * q.K, AF_POOL_BLOCKS));
    const dim3 gpix(af_grid(((long long)q.B * q.N + 255) / 256, AF_POOL_BLOCKS));
    AF_SWITCH_SM(sm, AF_SWITCH_CM(cm, (launch_pool<SM, CM>(vec, gpool, gpix, st, t1, t2, s1, s2, pa, pb, ia, ib, spart, q))));
    if (int rc = check_launch("attn_fuse pool")) return rc;
    if (p.ch) {
        const dim3 gfin(af_grid(((long long)q.B * q.C + AF_WAVES - 1) / AF_WAVES, AF_POOL_BLOCKS));
        if (p.cmax) hipLaunchKernelGGL(af_max_final_kernel, gfin, dim3(256), 0, st, pa, pb, ia, ib, c1, c2, ci1, ci2, q);
        else hipLaunchKernelGGL(af_sum_final_kernel<true>, gfin, dim3(256), 0, st, pa, pb, c1, c2, q);
        if (int rc = check_launch("attn_fuse pool final")) return rc;
    }
    const dim3 gel(af_grid((long long)q.B * q.C * q.ntiles, AF_ELEM_BLOCKS));
    AF_SWITCH_MODE(mode, (launch_join<MODE>(vec, gel, st, t1, t2, s1, s2, c1, c2, out, q)));
    return check_launch("attn_fuse join");
}

extern "C" int mmif_attn_fuse_bwd(const float* t1, const float* t2, const float* s1, const float* s2, const float* c1, const float* c2,
                                  const int32_t* ci1, const int32_t* ci2, const float* g, float* dt1, float* dt2, int32_t n, int32_t c, int32_t h, int32_t w,
                                  int32_t mode, int32_t spatial_mode, int32_t channel_mode, void* workspace, size_t workspace_bytes, void* stream) {
    AfGeo q;
    AfPlan p;
    if (int rc = af_check("mmif_attn_fuse_bwd", n, c, h, w, mode, spatial_mode, channel_mode, q, p)) return rc;
    MMIF_REQUIRE(t1 != nullptr && t2 != nullptr && g != nullptr && dt1 != nullptr && dt2 != nullptr && workspace != nullptr,
                 "mmif_attn_fuse_bwd: null pointer");
    if (int rc = af_check_pools("mmif_attn_fuse_bwd", p, s1, s2, c1, c2, ci1, ci2)) return rc;
    if (workspace_bytes < p.bytes) {
        set_error("mmif_attn_fuse_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.bytes);
        return MMIF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pa = (float*)(ws + p.off_pa);
    float* pb = (float*)(ws + p.off_pb);
    float* ds1 = (float*)(ws + p.off_ds1);
    float* ds2 = (float*)(ws + p.off_ds2);
    int* aux1 = (int*)(ws + p.off_aux1);
    int* aux2 = (int*)(ws + p.off_aux2);
    float* dc1 = (float*)(ws + p.off_dc1);
    float* dc2 = (float*)(ws + p.off_dc2);
    const bool vec = q.N % 4 == 0 && af_aligned({t1, t2, g, dt1, dt2, s1, s2, workspace});
    const int sm = p.sp ? spatial_mode : -1, cm = p.ch ? channel_mode : -1;
    const int aux = p.aux ? spatial_mode : 0;
    float* spart = (float*)(ws + p.off_spart);
    const dim3 gpool(af_grid((long long)q.B * q.ntiles * q.K, AF_POOL_BLOCKS));
    const dim3 gpix(af_grid(((long long)q.B * q.N + 255) / 256, AF_POOL_BLOCKS));
    AF_SWITCH_MODE(mode, (launch_reduce_aux<MODE>(aux, vec, gpool, st, t1, t2, g, s1, s2, c1, c2, ds1, ds2, aux1, aux2, pa, pb, spart, gpix, q)));
    if (int rc = check_launch("attn_fuse bwd reduce")) return rc;
    if (p.ch) {
        const dim3 gfin(af_grid(((long long)q.B * q.C + AF_WAVES - 1) / AF_WAVES, AF_POOL_BLOCKS));
        hipLaunchKernelGGL(af_sum_final_kernel<false>, gfin, dim3(256), 0, st, pa, pb, dc1, dc2, q);
        if (int rc = check_launch("attn_fuse bwd reduce final")) return rc;
    }
    const dim3 gel(af_grid((long long)q.B * q.C * q.ntiles, AF_ELEM_BLOCKS));
    AF_SWITCH_MODE(mode, AF_SWITCH_SM(sm, AF_SWITCH_CM(cm, (launch_grad<MODE, SM, CM>(vec, gel, st, t1, t2, g, s1, s2, c1, c2, ci1, ci2, ds1, ds2, aux1, aux2,
                                                                                       dc1, dc2, dt1, dt2, q)))));
    return check_launch("attn_fuse bwd grad");
}
