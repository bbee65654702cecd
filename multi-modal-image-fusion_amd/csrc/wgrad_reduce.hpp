// The one fixed-order reduction of the weight gradients' per-block partial sums.
//
// Every weight-gradient kernel writes one partial per block (G of them, `stride` floats apart); a small second launch folds them into
// dW / db in a fixed order, without atomics, so results are bit-identical run to run.  This header holds that fold ONCE:
//   - partial_sum(): the fixed-order sum of one output's G partials;
//   - one small MAP type per partial layout: a POD of the layout's parameters (destinations included) whose slot(idx) says where output
//     idx of the walk sits in a partial (off, stride) and where its sum goes (dst).  off < 0: nothing to do for this idx; dst == nullptr:
//     summed but not stored (a bias gradient nobody asked for);
//   - wgrad_reduce<Map, SL>: the one __global__ kernel (64 outputs x SL slices per block), wgrad_reduce_pair<Map, SL>: two jobs of one
//     layout in one launch (the two branches of the fused encoder backward), reduce_multi_kernel (csrc/reduce_defer.hip): the queued
//     jobs of a deferred backward pass in one launch;
//   - wgrad_reduce_launch(): the host launcher (slice count by the map's rule, deferral when a queue is open).
//
// INVARIANT: the bits of an output depend only on its (partial, off, stride, G, sl).  The grid shape, which thread owns which output
// and which of the three kernels runs the sum are free -- which is why the deferred launch and the pair launch match the single ones
// bit for bit (tests/test_gpu_wgrad_bits.py holds every layout to recorded bits).
//
// The per-block partial size of every layout (PER / per()) is defined here, next to its map; producers and workspace-size functions
// use that definition.  tools/check_wgrad_maps.cpp walks every map on the host: all of dW / db produced exactly once, off in [0, stride).
//
// NOT on this sum, on purpose: wgrad_reduce_kernel (csrc/conv_valu.hip), gconv_wg_reduce (csrc/conv_general.hip), pairconv_wgrad_reduce
// (csrc/pair.hip) and norm_chan_reduce_kernel (csrc/norm.hip) add serially or in an order of their own; moving them here would change
// their results' bits.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mmif {

// ---------------------------------------------------------------- the sum
// Thread vt of a (virtual) block of 64 outputs x sl slices (64 * sl threads, its red[sl][64] rows at `red`): slice s of output vt & 63
// walks g = s, s + sl, ... with 4 independent load chains (s0..s3 over g, g + sl, g + 2 sl, g + 3 sl, then a tail into s0), i.e. 4 sl
// loads of one output in flight and G / (4 sl) dependent round trips (the partials were written by other XCDs: ~1-2 us each; with 4
// slices a G = 256 reduce ran 16 of them: 8-14 us per launch, seven launches per train step).  Returns the sum in the slice-0 threads;
// EVERY thread of the block must call it (off < 0: contributes nothing).  sl = 4 (256 threads) for short partial lists (G <= 64), where
// 16 slices only add waves.  Callers with a compile-time slice count pass a constant.
constexpr int RED_SLICES = 16;
__device__ inline float partial_sum(const float* __restrict__ partial, long long off, long long stride, int G, int sl, int vt, float (*red)[64]) {
    const int o_local = vt & 63, slice = vt >> 6;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (off >= 0) {
        int g = slice;
        for (; g + 3 * sl < G; g += 4 * sl) {
            s0 += partial[g * stride + off];
            s1 += partial[(g + sl) * stride + off];
            s2 += partial[(g + 2 * sl) * stride + off];
            s3 += partial[(g + 3 * sl) * stride + off];
        }
        for (; g < G; g += sl) s0 += partial[g * stride + off];
    }
    red[slice][o_local] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    float t = 0.f;
    if (slice == 0) {
#pragma unroll
        for (int q = 0; q < sl; q += 4) t += (red[q][o_local] + red[q + 1][o_local]) + (red[q + 2][o_local] + red[q + 3][o_local]);
    }
    return t;
}

// ---------------------------------------------------------------- the maps
struct RedSlot { long long off, stride; float* dst; };

// Every map has: n() outputs in its walk (the launch covers cdiv(n, 64) * 64 indices), slot(idx), SL (slices; 0 = by G: > 64 ? 16 : 4)
// and NAME (the launch's name in error messages).  The grouped maps walk dW's order, then db; the x3 maps walk the PARTIAL's order
// (register-major tiles: 64 consecutive threads read 64 consecutive floats of every block's partial) and scatter.

// dW[cout][cin][KK] | db[cout] from partials of (input group of ICW channels) x (output group of OCW channels) blocks, each
// dW[OCW][ICW][KK] | db[OCW]; the bias sums live behind the weights of input group 0.  OCG_OUTER: group index icg + n_icg * ocg, else
// icg * n_ocg + ocg.
constexpr int grouped_per(int icw, int ocw, int kk) { return ocw * icw * kk + ocw; }      // floats of one block partial
template <int ICW, int OCW, int KK, bool OCG_OUTER>
struct grouped_wgrad_map {
    static constexpr int PER = grouped_per(ICW, OCW, KK);
    float* dw;
    float* db;
    int cin, cout, n_icg, n_ocg;
    __host__ __device__ int n() const { return cout * cin * KK + cout; }
    __host__ __device__ int group(int icg, int ocg) const { return OCG_OUTER ? icg + n_icg * ocg : icg * n_ocg + ocg; }
    __host__ __device__ RedSlot slot(int idx) const {
        const int total_w = cout * cin * KK;
        RedSlot s = {-1, (long long)n_icg * n_ocg * PER, nullptr};
        if (idx < total_w) {
            const int tap = idx % KK, c = (idx / KK) % cin, o = idx / (KK * cin);
            s.off = (long long)group(c / ICW, o / OCW) * PER + ((o % OCW) * ICW + (c % ICW)) * KK + tap;
            s.dst = dw + idx;
        } else if (idx < total_w + cout) {
            const int o = idx - total_w;
            s.off = (long long)group(0, o / OCW) * PER + OCW * ICW * KK + (o % OCW);
            s.dst = db != nullptr ? db + o : nullptr;
        }
        return s;
    }
};
// (named after the kernels they replace: a profile shows wgrad_reduce<mmif::wgrad_dma_reduce, 16> and so on)
template <int KS, int MFW, int ICF = 1>
struct wgrad_mfma_reduce : grouped_wgrad_map<16 * ICF, MFW * 16, KS * KS, false> {      // wgrad_mfma_kernel<KS, MFW, ., ICF>
    static constexpr int SL = 4;
    static constexpr const char* NAME = "wgrad_mfma_reduce";
};
struct wgrad_dma_reduce : grouped_wgrad_map<64, 64, 9, true> {                          // wgrad_dma_kernel (64 x 64 channel pairs, 3x3)
    static constexpr int SL = 0;
    static constexpr const char* NAME = "wgrad_dma_reduce";
};
template <int KS>
struct image_in_wgrad_reduce : grouped_wgrad_map<1, 16, KS * KS, true> {                // image_in_wgrad_kernel (cin = 1)
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "image_in_wgrad_reduce";
};
template <int KS>
struct image_out_wgrad_reduce : grouped_wgrad_map<16, 1, KS * KS, true> {               // image_out_wgrad_kernel, image_out_bwd16_kernel (cout = 1)
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "image_out_wgrad_reduce";
};
constexpr int WD_PER = wgrad_dma_reduce::PER;                    // dW[64 oc][64 ic][9], db[64]
constexpr int IB_PER = image_out_wgrad_reduce<3>::PER;           // dW[16][9], db

// partials in dW's natural layout ([cout][cin][3][3] then [cout]): taprow_wgrad_kernel, bwd_pair_kernel / bwd_pair_dma_kernel
struct taprow_wgrad_reduce {
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "wgrad_taprow_reduce";
    float* dw;
    float* db;
    int n_w, cout;
    static constexpr size_t per(int cin, int cout) { return (size_t)cout * cin * 9 + cout; }
    __host__ __device__ int n() const { return n_w + cout; }
    __host__ __device__ RedSlot slot(int idx) const {
        RedSlot s = {-1, n_w + cout, nullptr};
        if (idx < n_w + cout) {
            s.off = idx;
            s.dst = idx < n_w ? dw + idx : (db != nullptr ? db + (idx - n_w) : nullptr);
        }
        return s;
    }
};

// wgrad_x3_kernel: npairs x per(taps) floats per block, each pair [tile][reg 16][lane 64] | db[64]
struct wgrad_x3_reduce {
    static constexpr int SL = 0;
    static constexpr const char* NAME = "wgrad_x3_reduce";
    float* dw;
    float* db;
    int cin, cout, n_icg, n_ocg, taps;
    static constexpr int per(int taps) { return 64 * 64 * taps + 64; }
    __host__ __device__ int n() const { return n_icg * n_ocg * per(taps); }
    __host__ __device__ RedSlot slot(int idx) const {
        const int XW_PER = per(taps), npairs = n_icg * n_ocg;
        const int pair = idx / XW_PER, e = idx - pair * XW_PER;
        const int icg = pair % n_icg, ocg = pair / n_icg;
        RedSlot s = {-1, (long long)npairs * XW_PER, nullptr};
        if (pair >= npairs) return s;
        if (e < 64 * 64 * taps) {
            const int ln = e & 63, r = (e >> 6) & 15, tile = e >> 10;
            int mt, jt, tap;
            if (taps == 1) { mt = tile >> 1; jt = tile & 1; tap = 0; }
            else { const int u = tile % 3, v = (tile / 3) % 3, mj = tile / 9; mt = mj >> 1; jt = mj & 1; tap = u * 3 + v; }
            const int o = ocg * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), c = icg * 64 + jt * 32 + (ln & 31);
            if (o < cout && c < cin) { s.off = idx; s.dst = dw + ((long long)o * cin + c) * taps + tap; }
        } else if (icg == 0) {
            const int o = ocg * 64 + (e - 64 * 64 * taps);
            if (o < cout) { s.off = idx; s.dst = db != nullptr ? db + o : nullptr; }
        }
        return s;
    }
};

// the 768 floats of one (16 output x 16 input channel, tap column v) item of the thin / dense x3 kernels: [u][reg 4][lane 64]
__host__ __device__ inline void x3_item_elem(int e, int& item, int& o, int& cl, int& u) {
    const int ln = e & 63, r = (e >> 6) & 3;
    u = (e >> 8) % 3; item = e / 768;
    o = 4 * (ln >> 4) + r; cl = ln & 15;
}

// wgrad_x3_thin_kernel: [item 9][u][reg][lane] then db[16] (+ pad) behind all nine items, whatever the layer's item count; the walk is
// the layer's own items, then one block of 64 for the bias sums
constexpr int XT_PER = 9 * 768 + 64;
struct wgrad_x3_thin_reduce {
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "wgrad_x3_thin_reduce";
    float* dw;
    float* db;
    int cin, cout;
    __host__ __device__ int items() const { return cin <= 16 ? 3 : (cin <= 32 ? 6 : 9); }
    __host__ __device__ int n() const { return items() * 768 + 64; }
    __host__ __device__ RedSlot slot(int idx) const {
        const int e = idx < items() * 768 ? idx : 9 * 768 + (idx - items() * 768);
        RedSlot s = {-1, XT_PER, nullptr};
        if (e < 9 * 768) {
            int item, o, cl, u;
            x3_item_elem(e, item, o, cl, u);
            const int j = item / 3, v = item - 3 * j, c = 16 * j + cl;
            if (o < cout && c < cin) { s.off = e; s.dst = dw + ((long long)o * cin + c) * 9 + u * 3 + v; }
        } else if (e < 9 * 768 + 16) {
            const int o = e - 9 * 768;
            if (o < cout) { s.off = e; s.dst = db != nullptr ? db + o : nullptr; }
        }
        return s;
    }
};

// wgrad_x3_dense_kernel: the three DenseBlock convs (16 L -> 16 channels, L = 1..3) in one partial: items 0..2 | 3..8 | 9..17, db[3][16] (+ pad)
constexpr int XD_PER = 18 * 768 + 64;
struct wgrad_x3_dense_reduce {
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "wgrad_x3_dense_reduce";
    float* dw[3];
    float* db[3];
    __host__ __device__ int n() const { return XD_PER; }
    __host__ __device__ RedSlot slot(int e) const {
        RedSlot s = {-1, XD_PER, nullptr};
        if (e < 18 * 768) {
            int item, o, cl, u;
            x3_item_elem(e, item, o, cl, u);
            const int L = item < 3 ? 1 : (item < 9 ? 2 : 3), rel = item - (L == 1 ? 0 : (L == 2 ? 3 : 9));
            const int j = rel / 3, v = rel - 3 * j, c = 16 * j + cl;
            s.off = e;
            s.dst = dw[L - 1] + ((long long)o * (16 * L) + c) * 9 + u * 3 + v;
        } else if (e < 18 * 768 + 48) {
            const int L = (e - 18 * 768) / 16, o = (e - 18 * 768) % 16;
            s.off = e;
            s.dst = db[L] != nullptr ? db[L] + o : nullptr;
        }
        return s;
    }
};

// enc_wgrad_kernel, enc_bwd_fused_kernel: the DenseBlock encoder's four layers in one partial (floats):
// dW3 [16][48][9] | dW2 [16][32][9] | dW1 [16][16][9] | layer 0 [16 oc][16: taps 0..8, db0, 6 unused] | db1..3
constexpr int EW_OFF3 = 0, EW_OFF2 = 16 * 48 * 9, EW_OFF1 = EW_OFF2 + 16 * 32 * 9, EW_OFF0 = EW_OFF1 + 16 * 16 * 9;
constexpr int EW_OFFB = EW_OFF0 + 256, EW_PER = EW_OFFB + 48;
struct EwDst { float* dw0; float* db0; float* dw[3]; float* db[3]; };
struct enc_wgrad_reduce {
    static constexpr int SL = RED_SLICES;
    static constexpr const char* NAME = "enc_wgrad_reduce";
    EwDst D;
    __host__ __device__ int n() const { return EW_PER; }
    __host__ __device__ RedSlot slot(int idx) const {
        RedSlot s = {idx < EW_PER ? idx : -1, EW_PER, nullptr};
        if (idx < EW_OFF2) s.dst = D.dw[2] + idx;
        else if (idx < EW_OFF1) s.dst = D.dw[1] + (idx - EW_OFF2);
        else if (idx < EW_OFF0) s.dst = D.dw[0] + (idx - EW_OFF1);
        else if (idx < EW_OFFB) {
            const int oc = (idx - EW_OFF0) >> 4, k = (idx - EW_OFF0) & 15;
            if (k < 9) s.dst = D.dw0 + oc * 9 + k;
            else if (k == 9) s.dst = D.db0 != nullptr ? D.db0 + oc : nullptr;
            else s.off = -1;      // the unused floats of a layer-0 row
        } else if (idx < EW_PER) {
            const int L = (idx - EW_OFFB) >> 4, oc = (idx - EW_OFFB) & 15;
            s.dst = D.db[L] != nullptr ? D.db[L] + oc : nullptr;
        }
        return s;
    }
};

// ---------------------------------------------------------------- the kernels
// one job of the walk: sum output idx of `partial` (every thread of the virtual block calls this), store from the slice-0 threads
template <class Map>
__device__ inline void reduce_one(const Map& m, int idx, const float* __restrict__ partial, int G, int accumulate, int sl, int vt, float (*red)[64]) {
    const RedSlot s = m.slot(idx);
    const float t = partial_sum(partial, s.off, s.stride, G, sl, vt, red);
    if ((vt >> 6) == 0 && s.off >= 0 && s.dst != nullptr) *s.dst = accumulate ? *s.dst + t : t;
}

template <class Map, int SL>
__global__ __launch_bounds__(64 * SL) void wgrad_reduce(Map m, const float* __restrict__ partial, int G, int accumulate) {
    __shared__ float red[SL][64];
    reduce_one(m, blockIdx.x * 64 + (threadIdx.x & 63), partial, G, accumulate, SL, threadIdx.x, red);
}

// two jobs of one layout in ONE launch: blockIdx.y = job when every destination differs; with any destination in common (serial) job b
// must see what job a wrote, so the same thread runs the two sums one after the other -- the order of the two launches this replaces
template <class Map, int SL>
__global__ __launch_bounds__(64 * SL) void wgrad_reduce_pair(Map ma, const float* __restrict__ pa, int acc_a, Map mb, const float* __restrict__ pb, int acc_b,
                                                             int G, int serial) {
    __shared__ float red[SL][64];
    const int idx = blockIdx.x * 64 + (threadIdx.x & 63);
    if (serial || blockIdx.y == 0) reduce_one(ma, idx, pa, G, acc_a, SL, threadIdx.x, red);
    if (serial) __syncthreads();      // (red is reused by the second sum)
    if (serial || blockIdx.y == 1) reduce_one(mb, idx, pb, G, acc_b, SL, threadIdx.x, red);
}

// ---------------------------------------------------------------- deferred reduces (csrc/reduce_defer.hip)
// Every weight-gradient kernel of the decoder is followed by one of these reduce launches -- five launches of 5-9 us each per PFNetv1
// step, whatever little they do.  Between mmif_reduce_defer_begin() and mmif_reduce_defer_flush() the launches of the three layouts below
// are QUEUED instead (their partials go to slots of a caller-supplied arena, so that later producers do not overwrite them) and flush
// runs them as ONE launch: the same maps and the same sum, hence the same bits; one launch latency instead of five.
struct RedJob {
    enum Kind { DMA, TAPROW, IMAGE_OUT3, IMAGE_OUT1 };
    const float* partial;
    int kind, sl;          // slices of the job's sum (16: 1024-thread blocks, 4: 256-thread virtual blocks, four per launch block)
    int G, accumulate;
    int nvb;               // virtual blocks of 64 outputs
    union {
        wgrad_dma_reduce dma;
        taprow_wgrad_reduce taprow;
        image_out_wgrad_reduce<3> image_out3;
        image_out_wgrad_reduce<1> image_out1;
    };
    void set(const wgrad_dma_reduce& m) { kind = DMA; dma = m; }
    void set(const taprow_wgrad_reduce& m) { kind = TAPROW; taprow = m; }
    void set(const image_out_wgrad_reduce<3>& m) { kind = IMAGE_OUT3; image_out3 = m; }
    void set(const image_out_wgrad_reduce<1>& m) { kind = IMAGE_OUT1; image_out1 = m; }
};
template <class Map>
constexpr bool red_deferrable = std::is_same<Map, wgrad_dma_reduce>::value || std::is_same<Map, taprow_wgrad_reduce>::value ||
                                std::is_same<Map, image_out_wgrad_reduce<3>>::value || std::is_same<Map, image_out_wgrad_reduce<1>>::value;
// the buffer a producer should write its partials to: an arena slot while reductions are being deferred (and the arena / queue have room), else ws
float* defer_ws(float* ws, size_t bytes);
// queue the reduce of `partial` (true: queued, it runs at the next flush) -- only partials handed out by defer_ws() are queued
bool defer_push(const RedJob& job);

// ---------------------------------------------------------------- the launcher
// dW / db of map m = fixed-order sum of the G partials at `partial` (accumulate: onto what is there); queued instead while reductions are
// deferred and `partial` is the arena slot defer_ws() handed out last
template <class Map>
constexpr int red_slices(int G) { return (Map::SL == 0 ? G > 64 : Map::SL == 16) ? 16 : 4; }   // the map's slice rule
template <class Map>
int wgrad_reduce_launch(const Map& m, const float* partial, int G, int accumulate, hipStream_t st) {
    const int nvb = cdiv(m.n(), 64);
    const bool wide = red_slices<Map>(G) == 16;
    if constexpr (red_deferrable<Map>) {
        RedJob J;
        J.partial = partial; J.sl = wide ? 16 : 4; J.G = G; J.accumulate = accumulate; J.nvb = nvb;
        J.set(m);
        if (defer_push(J)) return MMIF_OK;
    }
    if constexpr (Map::SL == 0 || Map::SL == 16) {
        if (wide) hipLaunchKernelGGL((wgrad_reduce<Map, 16>), dim3(nvb), dim3(1024), 0, st, m, partial, G, accumulate);
    }
    if constexpr (Map::SL == 0 || Map::SL == 4) {
        if (!wide) hipLaunchKernelGGL((wgrad_reduce<Map, 4>), dim3(nvb), dim3(256), 0, st, m, partial, G, accumulate);
    }
    return check_launch(Map::NAME);
}

}  // namespace mmif
