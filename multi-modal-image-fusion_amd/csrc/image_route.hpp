// Which kernel an image-side layer call (Cin == 1 / Cout == 1; csrc/conv_image.hip, csrc/image_bwd.hip) launches, and on what grid: decided
// ONCE, here, by a pure host function of the call's geometry -- what conv_route.hpp is for the generic convs.  The launch sites launch what a
// plan says; mmif_conv2d_image_plan (csrc/conv_image.hip) answers from the same function, so the tests' case lists are checked against the
// dispatch itself.  No HIP runtime call in this header.
#pragma once
#include "wgrad_reduce.hpp"

namespace mmif {

constexpr int ITILE = 16;                        // tile edge of the one-tile-per-block kernels
constexpr int IB_TW = 32, IB_TH = 8;             // tile of the persistent 16-channel kernels: 8 rows x 32 columns = 256 pixels
constexpr int IMG_G = 512;                       // most partial sums a weight gradient writes (the workspace's block count)
constexpr int IF_MAXG = 1024;                    // image_out_fwd16_kernel: four persistent blocks per CU (39 registers, 25 KB of LDS each)

struct ImagePlan {
    enum Kernel { NONE, IN_FWD, IN_WGRAD, OUT_FWD16, OUT_FWD_TILED, OUT_FWD, OUT_DGRAD, OUT_WGRAD, OUT_BWD16 } kernel;
    int dtype, ks;
    int tiles_x, tiles_y;      // tiles per image row / column (weight gradients: 0)
    long long tiles;           // tiles in all; weight gradients: 256-pixel runs of the n h w pixels that size their grid
    int G;                     // blocks per channel block / image plane of the grid: dim3(G) persistent, dim3(tiles_x * tiles_y, n) tiled with
                               // G = their product, dim3(G, cb) weight gradients (= the partial sums per output that the reduce adds)
    int groups;                // weight gradients: 16-channel groups of a partial
    long long npix;            // weight gradients: n h w
    const char* why;           // NONE: what the call would say
};

// the persistent kernels' grid: at most `cap` blocks, a multiple of 8 from 8 on (the XCD-aware tile walk; fewer: the plain walk)
inline int image_persistent_grid(long long total, int cap) {
    int G = total < cap ? (int)total : cap;
    if (G >= 8) G = G / 8 * 8;
    return G;
}

inline bool image_out_bwd16_shape(int dtype, int cin, int ks, int h, int w) { return dtype == MMIF_BF16 && cin == 16 && ks == 3 && h >= 4 && w >= 4; }

// op: MMIF_IMAGE_*; c: the layer's channels (cout of the image_in entries, cin of the image_out ones); cb: channel blocks of the view the
// call is given (y / gy / x / gx); n, h, w: its logical extent; halo: its halo
inline ImagePlan image_plan(int op, int dtype, int c, int ks, int cb, int n, int h, int w, int halo) {
    ImagePlan p{};
    p.dtype = dtype; p.ks = ks;
    auto refuse = [&](const char* why) { p.kernel = ImagePlan::NONE; p.why = why; return p; };
    if (dtype != MMIF_F32 && dtype != MMIF_BF16) return refuse("dtype must be fp32 or bf16");
    if (ks != 1 && ks != 3) return refuse("ksize must be 1 or 3");
    if (c <= 0 || cb <= 0 || c > cb * 8) return refuse("the view's channel blocks do not hold the channels");
    if (n <= 0 || h <= 0 || w <= 0 || halo < 0) return refuse("bad extent");
    if (ks == 3 && (h < 2 || w < 2)) return refuse("reflect padding needs h,w >= 2");
    const bool wgrad = op == MMIF_IMAGE_IN_WGRAD || op == MMIF_IMAGE_OUT_WGRAD;
    if (wgrad) {
        // the kernels lay their partials out by the grid's channel blocks ((cb + 1) / 2 groups of 16), the reduce and the workspace by the channels
        if (cdiv(cb, 2) != cdiv(c, 16)) return refuse("the view's channel blocks do not match the channels' 16-channel groups");
        if (op == MMIF_IMAGE_OUT_WGRAD && halo != 0) return refuse("x must be an activation (halo 0)");
        if (op == MMIF_IMAGE_IN_WGRAD && halo > 1) return refuse("gy: halo 0 or 1");
        p.kernel = op == MMIF_IMAGE_IN_WGRAD ? ImagePlan::IN_WGRAD : ImagePlan::OUT_WGRAD;
        p.npix = (long long)n * h * w;
        p.tiles = (p.npix + 255) / 256;
        p.G = (int)(p.tiles < IMG_G ? p.tiles : IMG_G);
        p.groups = cdiv(c, 16);
        return p;
    }
    if (op == MMIF_IMAGE_OUT_BWD || (op == MMIF_IMAGE_OUT_FWD && ks == 3 && c == 16 && cb == 2 && dtype == MMIF_BF16)) {
        if (op == MMIF_IMAGE_OUT_BWD && !(image_out_bwd16_shape(dtype, c, ks, h, w) && cb == 2 && halo == 0))
            return refuse("bf16, 16 input channels (2 channel blocks, halo 0), 3x3, h, w >= 4 only");
        if (halo != 0) return refuse("bad input view");
        p.tiles_x = cdiv(w, IB_TW); p.tiles_y = cdiv(h, IB_TH);
        p.tiles = (long long)p.tiles_x * p.tiles_y * n;
        if (p.tiles >= (1ll << 31)) return refuse("too many tiles");
        p.kernel = op == MMIF_IMAGE_OUT_BWD ? ImagePlan::OUT_BWD16 : ImagePlan::OUT_FWD16;
        // backward: two persistent blocks per CU (512 = the workspace's block count); forward: four
        p.G = image_persistent_grid(p.tiles, op == MMIF_IMAGE_OUT_BWD ? IMG_G : IF_MAXG);
        return p;
    }
    if (op == MMIF_IMAGE_IN_FWD || op == MMIF_IMAGE_OUT_FWD) {
        if (halo != 0) return refuse(op == MMIF_IMAGE_IN_FWD ? "bad output view" : "bad input view");
        p.kernel = op == MMIF_IMAGE_IN_FWD ? ImagePlan::IN_FWD
                   : (ks == 3 && c == 16 && cb == 2) ? ImagePlan::OUT_FWD_TILED      // (fp32: the bf16 call went to the persistent kernel above)
                                                     : ImagePlan::OUT_FWD;
        p.tiles_x = cdiv(w, ITILE); p.tiles_y = cdiv(h, ITILE);
    } else if (op == MMIF_IMAGE_OUT_DGRAD) {
        if (halo < ks / 2) return refuse("gx needs halo >= ksize/2");
        p.kernel = ImagePlan::OUT_DGRAD;
        p.tiles_x = cdiv(w + 2 * halo, ITILE); p.tiles_y = cdiv(h + 2 * halo, ITILE);      // the STORED domain of gx
    } else {
        return refuse("bad op");
    }
    p.tiles = (long long)p.tiles_x * p.tiles_y * n;
    if (p.tiles >= (1ll << 31)) return refuse("too many tiles");
    p.G = (int)p.tiles;
    return p;
}

inline void image_plan_name(const ImagePlan& p, char* s, size_t n) {
    const char* t = p.dtype == MMIF_F32 ? "f32" : "bf16";
    switch (p.kernel) {
        case ImagePlan::IN_FWD: snprintf(s, n, "image_in_fwd<%s,%d>", t, p.ks); break;
        case ImagePlan::IN_WGRAD: snprintf(s, n, "image_in_wgrad<%s,%d>", t, p.ks); break;
        case ImagePlan::OUT_FWD16: snprintf(s, n, "image_out_fwd16"); break;
        case ImagePlan::OUT_FWD_TILED: snprintf(s, n, "image_out_fwd_tiled<%s>", t); break;
        case ImagePlan::OUT_FWD: snprintf(s, n, "image_out_fwd<%s,%d>", t, p.ks); break;
        case ImagePlan::OUT_DGRAD: snprintf(s, n, "image_out_dgrad<%s,%d>", t, p.ks); break;
        case ImagePlan::OUT_WGRAD: snprintf(s, n, "image_out_wgrad<%s,%d>", t, p.ks); break;
        case ImagePlan::OUT_BWD16: snprintf(s, n, "image_out_bwd16"); break;
        default: snprintf(s, n, "none"); break;
    }
}

}  // namespace mmif
