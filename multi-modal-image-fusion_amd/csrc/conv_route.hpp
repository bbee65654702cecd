// Which kernel a ConvLayer call launches, and on what grid: decided ONCE, here, by pure host functions of the call's geometry -- the bf16
// families and the fp32 split-operand ("x3") family.
//
// conv_mfma.hip / conv1x1.hip / enc_wgrad.hip / conv_x3.hip launch what a route says and nothing else; the `_supported` queries and
// mmif_conv2d_route (csrc/conv_api.hip) ask the same functions, so the tests and the engines see what the dispatch does.  No HIP runtime
// call in this header: the compute-unit count and the switches are arguments (the same arguments give the same route).
#pragma once
#include "common.hpp"
#include "enc_wgrad.hpp"

namespace mmif {

// ---------------------------------------------------------------- geometry the kernels and the routes share
constexpr int MT = 16;        // output tile edge
constexpr int DT_ROWS = 32;   // output tile rows of conv_dma_kernel (8 waves x 4)
constexpr int CHUNK_CB = 4;   // channel blocks per K chunk
// thin_conv_async_kernel
constexpr int TN_MAXCB = 6;                    // input channel blocks per tile (cin <= 48)
constexpr int TN_PL = 336;                     // granules per LDS plane (18x18 = 324 used); 5376 B = 0 mod 256
constexpr int TN_MAXKG = 2 * 36;               // k-group planes of two chunks
constexpr int TN_GROUPS = 3, TN_LOAD = 4, TN_MAXSLOTS = 8;   // 12 consumer + 4 loader waves = one 1024-thread block per CU
__host__ __device__ constexpr int tn_ring_bytes(int mf) { return mf == 1 ? 128 * 1024 : (mf == 2 ? 112 * 1024 : 96 * 1024); }
// the 64 -> 32 forward's geometry (thin_conv_async_kernel: two consumer groups, three tight slots of 324-granule planes)
constexpr int TNW_GROUPS = 2, TNW_PL = 324, TNW_MAXCB = 8, TNW_MAXP = (TNW_MAXCB * TNW_PL + 63) / 64 / TN_LOAD + 1;   // 41 pieces -> 11 per loader
constexpr int TNW_RING = 3 * ((TNW_MAXCB * TNW_PL + 63) / 64) * 1024;                                                  // 125 952 B
// conv1x1_stream_kernel
constexpr int C1_WAVES = 4;
constexpr int C1_PX = 32;   // pixels per wave item (two MFMA N tiles)
constexpr size_t C1_MAX_LDS = 128 * 1024;
constexpr int c1_waves_per_eu(int nmt) { return nmt <= 4 ? 4 : (nmt <= 8 ? 3 : 2); }   // by 16-row fragments of the output
inline size_t c1_lds_bytes(int nch, int m16p) { return (size_t)nch * 4 * m16p * 16 + (size_t)m16p * 4; }
constexpr int BP_MAXG = 512;   // blocks of bwd_pair_kernel
// the split-operand family (csrc/conv_x3.hip); the thin / dense partials' sizes XT_PER / XD_PER are in wgrad_reduce.hpp
constexpr int X3_TW = 32;                        // conv_x3_kernel: output tile columns; rows = 2 per wave (16 with 8 waves, 8 with 4)
constexpr int XW_TW = 16;                        // wgrad_x3_kernel: pixel-tile columns = the 16 pixels of one k-step
constexpr int XT_TH = 8, XT_TW = 16;             // wgrad_x3_thin_kernel / wgrad_x3_dense_kernel: pixel tile
__host__ __device__ constexpr int x3_mb(int n_out) { return n_out > 32 ? 2 : 1; }
inline int x3_nmb(int n_out) { return cdiv(n_out, 32 * x3_mb(n_out)); }
inline int x3_nch(int n_in) { return cdiv(cdiv(n_in, 8), 2); }

inline int pick_mf(int n_out) {
    const int fr = (n_out + 15) / 16;
    return fr <= 4 ? fr : 4;
}
inline int n_mblocks(int n_out) {
    const int fr = (n_out + 15) / 16, mf = pick_mf(n_out);
    return (fr + mf - 1) / mf;
}
inline int pick_mfw(int cout) { return cout <= 16 ? 1 : (cout <= 32 ? 2 : 4); }
// input-channel fragments per block of the register-staged wgrad: 1x1 layers with 64-row output groups take up to 4 (see the kernel)
inline int pick_icf(int ks, int cin, int cout) { return (ks == 1 && pick_mfw(cout) == 4) ? (cin > 32 ? 4 : (cin > 16 ? 2 : 1)) : 1; }

// ---------------------------------------------------------------- switches
// The mmif_debug_set_* switches (the tests' cross-checks; the kernels on either side of each give bit-identical results unless said) and
// $MMIF_WGRAD_TAPROW, read once where the process-wide instance is initialised (csrc/conv_mfma.hip).
struct ConvSwitches {
    int conv_dma = 1;             // mmif_debug_set_conv_dma: the DMA-staged / asynchronous kernels where they apply; 0 = register-staged only
    int thin_wide = 1;            // mmif_debug_set_thin_wide(0): decode.2's forward stays on the register-staged kernel
    int conv1x1_stream = 1;       // mmif_debug_set_conv1x1_stream(0): 1x1 layers stay on conv_mfma_kernel<1, ...>
    int wgrad_dma_blocks = 256;   // mmif_debug_set_wgrad_dma_blocks: persistent blocks of wgrad_dma_kernel (one per CU); fewer leave CUs to a
                                  // kernel running concurrently on another stream (the intra-step overlap experiment)
    int wgrad_ragged = 1;         // mmif_debug_set_ragged(0): wgrad_dma_kernel stages the padded planes of a ragged channel group too
    int wgrad_bias = 1;           // mmif_debug_set_wgrad_bias(0): every block of wgrad_dma_kernel sums the bias gradient, not only those of input
                                  // group 0 that the reduce reads
    int bwd_pair_dma = 1;         // mmif_debug_set_bwd_pair_dma(0): the register-staged bwd_pair_kernel
    int wgrad_taprow = 1;         // $MMIF_WGRAD_TAPROW=0: keep the per-input-group kernel (A/B timing)
};
extern ConvSwitches g_conv_switches;

inline int persistent_grid(int num_cus) {   // one persistent block per CU, a multiple of 8 (the XCD-aware tile walk), at least 8
    const int G = num_cus / 8 * 8;
    return G < 8 ? 8 : G;
}

// ---------------------------------------------------------------- forward / dgrad
enum class ConvForm { PLAIN, ONTO, DUP, WIDE_SIGNS };   // ONTO: accumulate operand from another tensor; DUP: + the masked copies (struct
                                                         // DupOut); WIDE_SIGNS: the dgrad half of bwd_wide, masks from the sign bytes
struct ConvRoute {
    enum Kernel { NONE, MFMA, CONV1X1_STREAM, CONV_DMA, THIN_WIDE, THIN_ASYNC } kernel;
    int ks, mf;
    int org;               // 1: the kernel folds the reflect halo itself (interior tiles + fold steps)
    int lmask;             // conv_dma_kernel: 0 consumers fetch the ReLU masks, 1 the loader waves stage them, 2 they stage the sign bytes
    bool dup;
    int tiles_x, tiles_y;
    long long items;       // tiles x images (x M-blocks where a block owns one); conv1x1_stream: 32-pixel runs
    int G;                 // blocks launched
};

// tin / tout: the operand read / written (dgrad: gy / gx); n_out = tout's channels; fold (dgrad): the caller wants fold_halo(gx) applied
// as well.  The 1x1 streaming kernel's conditions on the mask tensor follow from tout: the entry point has required x to match gx, halo 0.
// DUP and WIDE_SIGNS exist on conv_dma_kernel with org 1 only: NONE where that is not the route.  ONTO exists on THIN_ASYNC only; the
// route says where the call goes all the same (conv_mfma() words its refusal by it).
inline ConvRoute conv_route(bool dgrad, int ks, const TV& tin, const TV& tout, int n_out, uint64_t mask_bits, uint64_t accum_bits, bool fold,
                            ConvForm form, int num_cus, const ConvSwitches& sw) {
    ConvRoute r{};
    r.ks = ks;
    r.mf = pick_mf(n_out);
    r.org = (dgrad && (fold || form == ConvForm::DUP || form == ConvForm::WIDE_SIGNS) && ks == 3 && tout.halo == 1 && tout.h >= 4 && tout.w >= 4) ? 1 : 0;
    r.dup = form == ConvForm::DUP;
    const int nmb = n_mblocks(n_out), pgrid = persistent_grid(num_cus);
    const bool grad_in_ok = !dgrad || (tin.halo == 1 && tin.folded);   // an unfolded or halo-0 gy: only the register-staged kernel folds on load
    // 1x1 layers: the streaming kernel (csrc/conv1x1.hip: weights resident in LDS, B fragments straight from global memory)
    if (ks == 1 && form == ConvForm::PLAIN && sw.conv1x1_stream != 0 && accum_bits == 0) {
        const int m16p = nmb * r.mf * 16, nch = (tin.cb + 3) / 4;
        const bool same = tin.hs == tout.hs && tin.ws == tout.ws && tin.n == tout.n;          // same stored geometry: one linear walk
        if (same && (tin.halo == 0 || tin.folded) && m16p <= 256 && c1_lds_bytes(nch, m16p) <= C1_MAX_LDS &&
            tout.plane * 16 < (1ll << 31) &&                                                  // 32-bit in-plane offsets
            (long long)tin.n * cdiv(tin.plane, C1_PX) < (1ll << 31)) {
            r.kernel = ConvRoute::CONV1X1_STREAM;
            r.items = (long long)cdiv(tin.plane, C1_PX) * tin.n;
            int bpc = (int)((160 * 1024) / (c1_lds_bytes(nch, m16p) + 512));
            const int wpe = c1_waves_per_eu((n_out + 15) / 16);
            bpc = bpc < 1 ? 1 : (bpc > wpe ? wpe : bpc);
            r.G = num_cus * bpc;
            if (r.G > cdiv(r.items, C1_WAVES)) r.G = cdiv(r.items, C1_WAVES);
            if (r.G < 1) r.G = 1;
            return r;
        }
    }
    // the DMA-staged kernel: 3x3, 64-row M-blocks, input gradient already folded, tensors within 32-bit plane offsets
    if ((sw.conv_dma == 1 || form == ConvForm::WIDE_SIGNS) && ks == 3 && r.mf == 4 && grad_in_ok && tin.plane * 16 * CHUNK_CB < (1ll << 31)) {
        if ((form == ConvForm::DUP || form == ConvForm::WIDE_SIGNS) && r.org != 1) return r;
        r.kernel = ConvRoute::CONV_DMA;
        r.tiles_x = cdiv(tout.ws - 2 * r.org, MT);
        r.tiles_y = cdiv(tout.hs - 2 * r.org, DT_ROWS);
        r.items = (long long)r.tiles_x * r.tiles_y * tout.n * nmb;
        r.G = r.items < pgrid ? (int)r.items : pgrid;   // one persistent block per CU (150 KB of LDS each)
        // dgrad with ReLU masks and >= 2 chunks per tile: the loader waves stage the mask bits (-15 % on the dgrads against consumers fetching them)
        const bool lmask = dgrad && !r.dup && mask_bits != 0 && cdiv(tin.cb, CHUNK_CB) >= 2;
        r.lmask = lmask ? (form == ConvForm::WIDE_SIGNS ? 2 : 1) : 0;
        return r;
    }
    if (form == ConvForm::DUP || form == ConvForm::WIDE_SIGNS) return r;
    // thin layers: asynchronous loader / consumer kernel with resident weights (one M-block of <= 48 channels, <= 48 input
    // channels, a ring of at least GROUPS + 1 tile slots, at least two tiles per persistent block).  Measured (B=32 256x256,
    // vs conv_mfma_kernel<3,MF>): every dgrad -13 .. -21 %, forward with 32 / 48 outputs -14 % / -30 %; forward with 16 outputs
    // is +3 .. +16 % (the register-staged kernel runs 4 blocks per SIMD there), so that case stays on the old kernel.
    if (sw.conv_dma == 1 && ks == 3 && r.mf <= 3 && (dgrad || r.mf >= 2)) {
        const bool wide = sw.thin_wide == 1 && !dgrad && r.mf == 2 && tin.cb > TN_MAXCB && tin.cb <= TNW_MAXCB;   // the 64 -> 32 forward's geometry
        const int org = wide ? 0 : r.org;
        const int tiles_x = cdiv(tout.ws - 2 * org, MT), tiles_y = cdiv(tout.hs - 2 * org, MT);
        const long long ntiles = (long long)tiles_x * tiles_y * tout.n;
        bool ok;
        if (wide)
            ok = tin.plane * 16 * TNW_MAXCB < (1ll << 31) && TNW_RING / (cdiv(tin.cb * TNW_PL, 64) * 1024) >= TNW_GROUPS + 1;
        else
            ok = tin.cb <= TN_MAXCB && grad_in_ok && tin.plane * 16 * TN_MAXCB < (1ll << 31) &&
                 tn_ring_bytes(r.mf) / (cdiv(cdiv(tin.cb * TN_PL, 64), TN_LOAD) * TN_LOAD * 1024) >= TN_GROUPS + 1;
        if (ok && ntiles >= 2ll * pgrid && ntiles < (1ll << 31)) {
            r.kernel = wide ? ConvRoute::THIN_WIDE : ConvRoute::THIN_ASYNC;
            r.org = org;
            r.tiles_x = tiles_x; r.tiles_y = tiles_y; r.items = ntiles; r.G = pgrid;
            return r;
        }
    }
    r.kernel = ConvRoute::MFMA;
    r.org = 0;
    r.tiles_x = cdiv(tout.ws, MT);
    r.tiles_y = cdiv(tout.hs, MT);
    r.items = (long long)r.tiles_x * r.tiles_y * tout.n * nmb;   // one block per tile and M-block
    r.G = (int)r.items;
    return r;
}

// ---------------------------------------------------------------- weight gradient
// enc_wgrad.hip: single-layer "tap-row" kernel (whole x / g tile staged once per block)
inline bool wgrad_taprow_supported(int ks, int cin, int cout) {
    if (ks != 3 || cin % 16 || cout % 16) return false;
    const int nxb = cin / 16, ngb = cout / 16;
    return (ngb == 1 && nxb >= 1 && nxb <= 3) || (ngb == 2 && (nxb == 2 || nxb == 4));
}
inline bool wgrad_dma_shape(int ks, int cin, int cout) {
    const long long padded = (long long)cdiv(cin, 64) * 64 * cdiv(cout, 64) * 64;
    return ks == 3 && cin % 8 == 0 && cout % 8 == 0 && (long long)cin * cout * 10 >= padded * 6;
}
inline int wgrad_dma_G(int cin, int cout, int blocks = 256) {   // tile groups per (icg, ocg) pair: about one persistent block per CU in total
    const int npairs = cdiv(cin, 64) * cdiv(cout, 64);
    int G = blocks / npairs;
    if (G >= 8) G = G / 8 * 8;   // multiples of 8 keep the blocks that share tiles on one XCD
    return G < 1 ? 1 : G;
}
// tile groups per (icg, ocg) pair of the register-staged wgrad.  The grid is G * nb persistent blocks; it must fit the resident
// capacity in ONE round (3 blocks/CU at MFW = 1 -- 136 VGPRs --, else 2; 256 CUs): 1032 blocks on 768 slots ran a second round
// at 34 % occupancy.
inline int wgrad_mfma_G(int cin, int cout, int icf = 1) {
    const int mfw = pick_mfw(cout);
    const int nb = cdiv(cin, 16 * icf) * cdiv(cout, mfw * 16);
    const int capacity = 256 * (mfw == 1 ? 3 : 2);
    int G = capacity / nb / 8 * 8;
    if (G > 512) G = 512;   // (768 blocks for a single pair measured 8 % slower than 512)
    return G < 8 ? 8 : G;
}

struct WgradRoute {
    enum Kernel { NONE, DMA, TAPROW, MFMA } kernel;
    int ks, mfw, ksplit, icf;     // MFMA: wgrad_mfma_kernel<ks, mfw, ksplit, icf>
    int tiles_x, tpi, total;      // 16 x 16 tiles: per row, per image, in all
    int n_icg, n_ocg;             // channel groups (DMA: 64 x 64, MFMA: 16 icf x 16 mfw); the grid is G * n_icg * n_ocg blocks
    int G;                        // partials the reduce sums: tile groups per channel-group pair, every one owning at least one tile
    int slices;                   // of the reduce
};
// wide: the weight-gradient half of bwd_wide -- wgrad_dma_kernel (it leaves the sign bytes) or nothing
inline WgradRoute wgrad_route(int ks, int cin, int cout, const TV& tx, const TV& tg, int num_cus, const ConvSwitches& sw, bool wide = false) {
    (void)num_cus;   // (these grids are sized for the part's 256 compute units, not the device's)
    WgradRoute r{};
    r.ks = ks;
    r.tiles_x = cdiv(tx.w, MT);
    r.tpi = r.tiles_x * cdiv(tx.h, MT);
    r.total = r.tpi * tx.n;
    r.n_icg = r.n_ocg = 1;
    if ((sw.conv_dma == 1 || wide) && wgrad_dma_shape(ks, cin, cout) && tg.halo == 1 && tg.folded && tx.plane * 16 * 8 < (1ll << 31) &&
        tg.plane * 16 * 8 < (1ll << 31)) {
        r.kernel = WgradRoute::DMA;
        r.n_icg = cdiv(cin, 64); r.n_ocg = cdiv(cout, 64);
        r.G = wgrad_dma_G(cin, cout, sw.wgrad_dma_blocks);   // (the workspace is sized for the full grid)
        if (r.G > r.total) r.G = r.total;
        r.slices = red_slices<wgrad_dma_reduce>(r.G);
    } else if (wide) {
        return r;
    } else if (sw.wgrad_taprow == 1 && wgrad_taprow_supported(ks, cin, cout) && (tg.halo == 0 || tg.folded) && tx.halo == 0) {
        r.kernel = WgradRoute::TAPROW;
        r.G = r.total < EW_MAXG ? r.total : EW_MAXG;
        r.slices = red_slices<taprow_wgrad_reduce>(r.G);
    } else {
        r.kernel = WgradRoute::MFMA;
        r.mfw = pick_mfw(cout);
        r.ksplit = r.mfw == 1 ? 4 : 2;
        r.icf = pick_icf(ks, cin, cout);
        r.n_icg = cdiv(cin, 16 * r.icf); r.n_ocg = cdiv(cout, r.mfw * 16);
        r.G = wgrad_mfma_G(cin, cout, r.icf);
        if (r.G > r.total) r.G = r.total;   // (no longer a multiple of 8: the kernel falls back to the plain block order)
        r.slices = red_slices<wgrad_mfma_reduce<3, 1>>(r.G);
    }
    return r;
}

// ---------------------------------------------------------------- bwd_pair: dgrad + wgrad of one thin 3x3 layer in one launch
inline bool bwd_pair_supported(int ks, int cin, int cout) { return ks == 3 && ((cin == 64 && cout == 32) || (cin == 32 && cout == 16)); }
struct PairRoute {
    enum Kernel { NONE, DMA, REG } kernel;   // tiles staged by LDS-DMA (bwd_pair_dma_kernel) or through registers (bwd_pair_kernel)
    int tiles_x, tpi, total;
    int G, slices;
};
inline PairRoute pair_route(int ks, int cin, int cout, const TV& tx, const TV& tg, int num_cus, const ConvSwitches& sw) {
    PairRoute r{};
    if (!bwd_pair_supported(ks, cin, cout)) return r;
    r.kernel = (sw.bwd_pair_dma == 1 && tg.halo == 1 && tg.folded) ? PairRoute::DMA : PairRoute::REG;
    r.tiles_x = cdiv(tx.w, MT);
    r.tpi = r.tiles_x * cdiv(tx.h, MT);
    r.total = r.tpi * tx.n;
    const int cap = (cin == 64 ? 1 : 2) * num_cus < BP_MAXG ? (cin == 64 ? 1 : 2) * num_cus : BP_MAXG;   // (the workspace holds BP_MAXG partials)
    r.G = r.total < cap ? r.total : cap;
    r.slices = red_slices<taprow_wgrad_reduce>(r.G);
    return r;
}

// ---------------------------------------------------------------- fp32 tensors: the split-operand ("x3") family (csrc/conv_x3.hip)
// The forward operand format (16 | 3 | 2, csrc/conv_x3.hip; dgrad: always 2) and $MMIF_X3 (`enabled`) are arguments like the compute units.
struct X3Route {
    int mb;                          // 0: not taken; else conv_x3_kernel<mb, dgrad, np, nw, rj, ks, f16, m16>
    int np, nw, rj, ks;
    bool f16, m16, dgrad;
    int org;                         // 1: interior tiles + in-tile fold steps, the halo ring stays untouched (zero: the fold-me call's contract)
    int n_out, nch, nmb;             // output channels, input chunks, M-blocks
    int tiles_x, tpi, total;         // 32 x (rj nw) tiles: per row, per image, in all
    int G;                           // persistent blocks
};
inline bool x3_grad_ok(const TV& t) { return t.halo == 0 || (t.halo == 1 && t.folded); }
inline bool x3_small(const TV& t) { return t.plane * 32 * 8 < (1ll << 32); }   // 8 planes addressed with 32-bit byte offsets
// forward: tin = x, tout = y;  dgrad: tin = gy (halo 0 or folded halo 1), tout = gx (the padded domain is written unless org = 1);
// want_fold (dgrad): the caller wants fold_halo(gx) applied and guarantees a zero halo ring on entry -- org says whether the kernel does it
inline X3Route x3_conv_route(bool dgrad, int ks, const TV& tin, const TV& tout, int n_out, int n_in, int fmt, bool want_fold, int num_cus, bool enabled) {
    X3Route r{};
    if (!enabled || (ks != 3 && ks != 1) || n_in < 1 || n_out < 1 || (dgrad && !x3_grad_ok(tin))) return r;
    if (n_out > 64 * 8) return r;   // mask / accum bits address 64 channel blocks
    if (!(ks == 1 || (tin.h >= 2 && tin.w >= 2)) || !x3_small(tin) || !x3_small(tout)) return r;
    const bool six = !dgrad && fmt == 3;
    r.mb = x3_mb(n_out); r.np = six ? 3 : 2; r.nw = 8; r.rj = 2; r.ks = ks;
    r.f16 = !dgrad && fmt == 16; r.dgrad = dgrad;
    if (ks == 3 && r.mb == 1) {
        // thin layers (<= 32 out, <= 64 in: the DenseBlock convs and the decoder's tail) have almost no MFMA work per tile and run at the
        // latency of ONE tile's loads per block: four-wave blocks (8-row tiles, 16-channel chunks, 42 KB of LDS, 146 VGPRs) put THREE
        // independent blocks on a CU: forward 16->16 102 -> 77 us, 32->16 161 -> 144, 48->16 258 -> 212, 64->32 348 -> 324; dgrad 16->16
        // 160 -> 123, 32->16 204 -> 175 (two blocks: half of that; four: over-subscribed, slower; the 64-out-channel kernels on four-wave
        // blocks: +-0).  <= 16 output channels: 16 x 16 x 32 MFMAs, K = two taps x 16 channels (no padded half tile)
        if (n_in <= 64 && !six) { r.nw = 4; r.m16 = n_out <= 16; }
        // one 32-channel accumulator tile per pixel row, so a wave takes FOUR rows (32 x 32 pixel tiles) in the 3-piece forward: the same
        // 216 MFMAs per wave and barrier as the 64-channel kernels for half the weight staging
        else if (six) r.rj = 4;
    }
    r.org = (dgrad && ks == 3 && !r.m16 && want_fold && tout.halo == 1 && tout.h >= 4 && tout.w >= 4) ? 1 : 0;
    r.n_out = n_out; r.nch = x3_nch(n_in); r.nmb = x3_nmb(n_out);
    r.tiles_x = cdiv(tout.ws - 2 * r.org, X3_TW);
    r.tpi = r.tiles_x * cdiv(tout.hs - 2 * r.org, r.rj * r.nw);
    r.total = r.tpi * tout.n;
    r.G = num_cus * (r.nw == 4 ? 3 : 1);   // four-wave blocks: three per CU (42 KB of LDS, < 168 VGPRs each; two: half the gain; four: over-subscribed)
    if (r.total < r.G) r.G = r.total;
    return r;
}

// Tile groups per 64 x 64 channel pair of wgrad_x3_kernel: about one persistent block per CU in total, never more than the workspace holds
inline int x3_wgrad_pairs(int cin, int cout) { return cdiv(cin, 64) * cdiv(cout, 64); }
inline int x3_wgrad_G_max(int cin, int cout) {   // a gfx950 part has at most 256 CUs
    const int G = 256 / x3_wgrad_pairs(cin, cout);
    return G < 1 ? 1 : G;
}
inline int x3_wgrad_G(int cin, int cout, int num_cus) {
    int G = num_cus / x3_wgrad_pairs(cin, cout);
    if (G >= 8) G &= ~7;
    if (G > x3_wgrad_G_max(cin, cout)) G = x3_wgrad_G_max(cin, cout);
    return G < 1 ? 1 : G;
}
inline size_t x3_wgrad_workspace_bytes(int cin, int cout, int ks) {   // (1x1: three k-split partials per block)
    if (ks != 1 && ks != 3) return 0;
    return (size_t)(ks == 1 ? 3 : 1) * x3_wgrad_G_max(cin, cout) * x3_wgrad_pairs(cin, cout) * wgrad_x3_reduce::per(ks * ks) * sizeof(float);
}
constexpr int XD_MAXG = 512;   // wgrad_x3_dense_kernel: two blocks per CU
inline int x3_dense_G(int total, int num_cus) {
    const int G = 2 * num_cus < XD_MAXG ? 2 * num_cus : XD_MAXG;
    return total < G ? total : G;
}

struct X3WgradRoute {
    enum Kernel { NONE, K1, THIN, THIN16, WIDE } kernel;   // wgrad_x3_kernel<8,8,8,1>, wgrad_x3_thin_kernel<nxc>, wgrad_x3_kernel<16,6,2,3> / <8,8,8,3>
    int nxc;                      // THIN: input channel blocks staged (2 | 4 | 6)
    int tiles_x, tpi, total;      // 8 x 16 pixel tiles (THIN16: 16 x 16): per row, per image, in all
    int n_icg, n_ocg;             // 64 x 64 channel groups; the grid is G * n_icg * n_ocg blocks (THIN: one group)
    int G;                        // tile groups launched per channel-group pair
    int red_G, slices;            // partials the reduce sums (1x1: three per block) and its slices
};
inline X3WgradRoute x3_wgrad_route(int ks, int cin, int cout, const TV& tx, const TV& tg, int num_cus, bool enabled) {
    X3WgradRoute r{};
    if (!enabled || (ks != 3 && ks != 1) || cin < 1 || cout < 1 || !x3_grad_ok(tg) || tx.halo != 0) return r;
    if (!(ks == 1 || (tx.h >= 2 && tx.w >= 2)) || !x3_small(tx) || !x3_small(tg)) return r;
    const bool thin = ks == 3 && cin <= 48 && cout <= 16;
    auto tiles = [&](int th, int tw) {
        r.tiles_x = cdiv(tx.w, tw);
        r.tpi = r.tiles_x * cdiv(tx.h, th);
        r.total = r.tpi * tx.n;
    };
    r.n_icg = r.n_ocg = 1;
    if (thin) {
        tiles(XT_TH, XT_TW);
        r.G = num_cus * (cin <= 16 ? 5 : (cin <= 32 ? 4 : 3));   // blocks per CU: what the registers (92 / 128 / 168) and the LDS (20 / 32 / 44 KB) allow
        if (r.total < r.G) r.G = r.total;
        if ((size_t)r.G * XT_PER * sizeof(float) <= x3_wgrad_workspace_bytes(cin, cout, 3)) {
            r.kernel = X3WgradRoute::THIN;
            r.nxc = cin <= 16 ? 2 : (cin <= 32 ? 4 : 6);
            r.red_G = r.G;
            r.slices = red_slices<wgrad_x3_thin_reduce>(r.red_G);
            return r;
        }
    }
    r.kernel = ks == 1 ? X3WgradRoute::K1 : (thin ? X3WgradRoute::THIN16 : X3WgradRoute::WIDE);
    tiles(thin ? 16 : 8, XW_TW);
    r.n_icg = cdiv(cin, 64); r.n_ocg = cdiv(cout, 64);
    r.G = x3_wgrad_G(cin, cout, num_cus);
    if (r.total < r.G) r.G = r.total;
    r.red_G = ks == 1 ? 3 * r.G : r.G;
    r.slices = red_slices<wgrad_x3_reduce>(r.red_G);
    return r;
}

// ---------------------------------------------------------------- names (tests/conv_cases.py REQUIRED_LABELS)
inline void route_name(const ConvRoute& r, char* s, size_t n) {
    switch (r.kernel) {
        case ConvRoute::MFMA: snprintf(s, n, "mfma<%d,%d>", r.ks, r.mf); break;
        case ConvRoute::CONV1X1_STREAM: snprintf(s, n, "conv1x1_stream"); break;
        case ConvRoute::CONV_DMA: snprintf(s, n, "conv_dma<L%d,org%d%s>", r.lmask, r.org, r.dup ? ",dup" : ""); break;
        case ConvRoute::THIN_WIDE: snprintf(s, n, "thin_wide"); break;
        case ConvRoute::THIN_ASYNC: snprintf(s, n, "thin_async<%d>", r.mf); break;
        default: snprintf(s, n, "none"); break;
    }
}
inline void route_name(const WgradRoute& r, char* s, size_t n) {
    switch (r.kernel) {
        case WgradRoute::DMA: snprintf(s, n, "wgrad_dma"); break;
        case WgradRoute::TAPROW: snprintf(s, n, "wgrad_taprow"); break;
        case WgradRoute::MFMA:
            if (r.ks == 1 && r.mfw == 4) snprintf(s, n, "wgrad_mfma<1,4,%d,%d>", r.ksplit, r.icf);
            else snprintf(s, n, "wgrad_mfma<%d,%d>", r.ks, r.mfw);
            break;
        default: snprintf(s, n, "none"); break;
    }
}
inline void route_name(const X3Route& r, char* s, size_t n) {   // one per code object: "x3<3,mb1,h16,nw4,m16>", "x3_dgrad<1,mb2>"
    if (r.mb == 0) { snprintf(s, n, "none"); return; }
    const char* fmt = r.dgrad ? "" : (r.f16 ? ",h16" : (r.np == 3 ? ",b3" : ",b2"));   // (the input gradient always reads two bf16 pieces)
    snprintf(s, n, "x3%s<%d,mb%d%s%s%s%s>", r.dgrad ? "_dgrad" : "", r.ks, r.mb, fmt, r.nw == 4 ? ",nw4" : "", r.m16 ? ",m16" : "", r.rj == 4 ? ",rj4" : "");
}
inline void route_name(const X3WgradRoute& r, char* s, size_t n) {
    switch (r.kernel) {
        case X3WgradRoute::K1: snprintf(s, n, "x3_wgrad<1>"); break;
        case X3WgradRoute::THIN: snprintf(s, n, "x3_wgrad_thin<%d>", r.nxc); break;
        case X3WgradRoute::THIN16: snprintf(s, n, "x3_wgrad_thin16"); break;
        case X3WgradRoute::WIDE: snprintf(s, n, "x3_wgrad<3>"); break;
        default: snprintf(s, n, "none"); break;
    }
}
inline void route_name(const PairRoute& r, char* s, size_t n) {
    snprintf(s, n, "%s", r.kernel == PairRoute::DMA ? "bwd_pair" : (r.kernel == PairRoute::REG ? "bwd_pair<reg>" : "none"));
}

}  // namespace mmif
