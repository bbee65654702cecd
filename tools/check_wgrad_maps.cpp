// Host-only check of the reduce maps of csrc/wgrad_reduce.hpp (make -C multi-modal-image-fusion_amd/csrc check-maps; built with the address
// and undefined-behaviour sanitizers; no HIP call, no GPU).  A map's slot(idx) tells the reduce kernel where to read (off, stride) and
// where to write (dst); an off outside a partial is a wild device read.  For every map, at the channel / kernel-size combinations of
// tests/wgrad_bits_cases.py plus the ragged ones each layout allows, walk idx over the launcher's grid (cdiv(n, 64) * 64) and require:
//   - every dW / db element is produced exactly once, and db not at all when it is null;
//   - every off is in [0, stride);
//   - no two outputs share an off;
//   - wgrad_dma_reduce (the single and the deferred launch run the same map): db is read from the blocks of input group 0 only.
#include <stdio.h>

#include <vector>

#include "wgrad_reduce.hpp"

using namespace mmif;

static int g_failed = 0, g_cases = 0;

struct Dest { float* base; size_t n; };   // a destination array the map may write (base == nullptr: not wanted)

template <class Map>
static void check(const char* what, const Map& m, const std::vector<Dest>& dests) {
    ++g_cases;
    std::vector<std::vector<int>> hits;
    for (const Dest& d : dests) hits.emplace_back(d.base != nullptr ? d.n : 0, 0);
    std::vector<char> seen;
    int bad = 0;
    const long long walk = (long long)((m.n() + 63) / 64) * 64;
    for (long long idx = 0; idx < walk; ++idx) {
        const RedSlot s = m.slot((int)idx);
        if (s.off < 0) {
            if (s.dst != nullptr && bad++ < 5) printf("  %s: idx %lld has a destination but no offset\n", what, idx);
            continue;
        }
        if (s.stride <= 0 || s.off >= s.stride) {
            if (bad++ < 5) printf("  %s: idx %lld: off %lld outside [0, %lld)\n", what, idx, s.off, s.stride);
            continue;
        }
        if (seen.empty()) seen.assign((size_t)s.stride, 0);
        if (seen.size() != (size_t)s.stride) { if (bad++ < 5) printf("  %s: idx %lld: stride changes within a map\n", what, idx); continue; }
        if (seen[(size_t)s.off]++ && bad++ < 5) printf("  %s: idx %lld: off %lld read for a second output\n", what, idx, s.off);
        if (s.dst == nullptr) continue;
        bool found = false;
        for (size_t d = 0; d < dests.size() && !found; ++d) {
            if (dests[d].base == nullptr || s.dst < dests[d].base || s.dst >= dests[d].base + dests[d].n) continue;
            ++hits[d][(size_t)(s.dst - dests[d].base)];
            found = true;
        }
        if (!found && bad++ < 5) printf("  %s: idx %lld: destination outside every dW / db\n", what, idx);
    }
    for (size_t d = 0; d < dests.size(); ++d)
        for (size_t i = 0; i < hits[d].size(); ++i)
            if (hits[d][i] != 1 && bad++ < 5) printf("  %s: destination %zu element %zu produced %d times\n", what, d, i, hits[d][i]);
    if (bad) { ++g_failed; printf("FAIL %s (%d findings)\n", what, bad); }
}

// dW[cout][cin][kk] + db[cout] maps, with and without db
template <class Map, class Make>
static void check_conv(const char* name, int cin, int cout, int kk, Make make) {
    std::vector<float> dw((size_t)cout * cin * kk), db(cout);
    char what[128];
    for (int with_db = 0; with_db < 2; ++with_db) {
        snprintf(what, sizeof(what), "%s cin %d cout %d kk %d db %d", name, cin, cout, kk, with_db);
        float* pdb = with_db ? db.data() : nullptr;
        check<Map>(what, make(dw.data(), pdb), {{dw.data(), dw.size()}, {pdb, db.size()}});
    }
}
static int cdiv_(int a, int b) { return (a + b - 1) / b; }

// The grouped maps read the bias sums from the blocks of input group 0 alone, so the blocks of the other groups need not write theirs
// (wgrad_dma_kernel and wgrad_mfma_kernel compute none there): no idx of the walk may read a bias slot of a group icg > 0.
template <class Map>
static void check_bias_slots(const char* name, const Map& m, int bias_off) {   // bias_off: where the bias sums start in a block partial
    ++g_cases;
    int bad = 0, from_group0 = 0;
    const long long walk = (long long)((m.n() + 63) / 64) * 64;
    for (long long idx = 0; idx < walk; ++idx) {
        const RedSlot s = m.slot((int)idx);
        if (s.off < 0) continue;
        const long long grp = s.off / Map::PER, e = s.off % Map::PER;
        if (e < bias_off) continue;
        // (group = icg + n_icg * ocg or icg * n_ocg + ocg: recover icg by asking the map)
        bool is_group0 = false;
        for (int ocg = 0; ocg < m.n_ocg; ++ocg) is_group0 |= grp == m.group(0, ocg);
        if (is_group0) ++from_group0;
        else if (bad++ < 5) printf("  %s: idx %lld reads bias slot %lld of block group %lld, an input group > 0\n", name, idx, e - bias_off, grp);
    }
    if (from_group0 != m.cout && bad++ < 5) printf("  %s: %d bias sums read from input group 0, %d output channels\n", name, from_group0, m.cout);
    if (bad) { ++g_failed; printf("FAIL %s: bias slots (%d findings)\n", name, bad); }
}

template <int KS, int MFW, int ICF>
static void check_mfma(int cin, int cout) {
    using M = wgrad_mfma_reduce<KS, MFW, ICF>;
    check_conv<M>("wgrad_mfma_reduce", cin, cout, KS * KS, [&](float* dw, float* db) { return M{{dw, db, cin, cout, cdiv_(cin, 16 * ICF), cdiv_(cout, MFW * 16)}}; });
}
template <int KS>
static void check_image(int c) {
    using I = image_in_wgrad_reduce<KS>;
    using O = image_out_wgrad_reduce<KS>;
    check_conv<I>("image_in_wgrad_reduce", 1, c, KS * KS, [&](float* dw, float* db) { return I{{dw, db, 1, c, 1, cdiv_(c, 16)}}; });
    check_conv<O>("image_out_wgrad_reduce", c, 1, KS * KS, [&](float* dw, float* db) { return O{{dw, db, c, 1, cdiv_(c, 16), 1}}; });
}

int main() {
    // wgrad_dma: multiples of 8, ragged last groups included
    const int dma[][2] = {{64, 64}, {128, 64}, {64, 128}, {192, 128}, {64, 136}, {136, 64}, {120, 56}, {8, 8}, {200, 72}};
    for (auto& c : dma) {
        check_conv<wgrad_dma_reduce>("wgrad_dma_reduce", c[0], c[1], 9,
                                     [&](float* dw, float* db) { return wgrad_dma_reduce{{dw, db, c[0], c[1], cdiv_(c[0], 64), cdiv_(c[1], 64)}}; });
        // (the deferred launch of csrc/reduce_defer.hip runs this same map: one answer for both)
        std::vector<float> dw((size_t)c[1] * c[0] * 9);
        check_bias_slots("wgrad_dma_reduce", wgrad_dma_reduce{{dw.data(), nullptr, c[0], c[1], cdiv_(c[0], 64), cdiv_(c[1], 64)}}, 64 * 64 * 9);
    }
    {   // NestFuse's widest layer: five input groups
        std::vector<float> dw((size_t)152 * 304 * 9);
        check_bias_slots("wgrad_dma_reduce 304 -> 152", wgrad_dma_reduce{{dw.data(), nullptr, 304, 152, 5, 3}}, 64 * 64 * 9);
    }
    // wgrad_mfma: every instantiation the library launches; any channel count
    const int any[][2] = {{16, 16}, {8, 8}, {24, 40}, {48, 16}, {33, 7}, {64, 32}, {100, 70}, {1, 1}};
    for (auto& c : any) {
        check_mfma<3, 1, 1>(c[0], c[1]); check_mfma<3, 2, 1>(c[0], c[1]); check_mfma<3, 4, 1>(c[0], c[1]);
        check_mfma<1, 1, 1>(c[0], c[1]); check_mfma<1, 2, 1>(c[0], c[1]); check_mfma<1, 4, 1>(c[0], c[1]);
        check_mfma<1, 4, 2>(c[0], c[1]); check_mfma<1, 4, 4>(c[0], c[1]);
    }
    for (int c : {1, 8, 16, 17, 24, 64, 100}) { check_image<3>(c); check_image<1>(c); }
    // taprow / fused pair backward: natural layout
    const int tap[][2] = {{16, 16}, {32, 16}, {48, 16}, {32, 32}, {64, 32}};
    for (auto& c : tap)
        check_conv<taprow_wgrad_reduce>("taprow_wgrad_reduce", c[0], c[1], 9,
                                        [&](float* dw, float* db) { return taprow_wgrad_reduce{dw, db, c[1] * c[0] * 9, c[1]}; });
    // x3 wide: 3x3 and 1x1, ragged groups
    const int x3[][2] = {{64, 64}, {128, 64}, {64, 32}, {56, 64}, {72, 40}, {136, 64}, {8, 8}, {48, 32}};
    for (auto& c : x3)
        for (int taps : {9, 1})
            check_conv<wgrad_x3_reduce>("wgrad_x3_reduce", c[0], c[1], taps, [&](float* dw, float* db) {
                return wgrad_x3_reduce{dw, db, c[0], c[1], cdiv_(c[0], 64), cdiv_(c[1], 64), taps};
            });
    // x3 thin: cin <= 48, cout <= 16
    const int thin[][2] = {{16, 16}, {32, 16}, {48, 16}, {8, 8}, {24, 16}, {40, 8}, {48, 1}, {1, 16}};
    for (auto& c : thin)
        check_conv<wgrad_x3_thin_reduce>("wgrad_x3_thin_reduce", c[0], c[1], 9,
                                         [&](float* dw, float* db) { return wgrad_x3_thin_reduce{dw, db, c[0], c[1]}; });
    // the two encoder layouts: fixed shapes; db of any layer may be null
    for (int mask = 0; mask < 16; ++mask) {
        std::vector<float> dw0(16 * 9), dw1(16 * 16 * 9), dw2(16 * 32 * 9), dw3(16 * 48 * 9), db[4] = {std::vector<float>(16), std::vector<float>(16), std::vector<float>(16), std::vector<float>(16)};
        float* pdb[4];
        for (int i = 0; i < 4; ++i) pdb[i] = (mask >> i & 1) ? db[i].data() : nullptr;
        char what[64];
        snprintf(what, sizeof(what), "enc_wgrad_reduce db mask %d", mask);
        check(what, enc_wgrad_reduce{{dw0.data(), pdb[0], {dw1.data(), dw2.data(), dw3.data()}, {pdb[1], pdb[2], pdb[3]}}},
              {{dw0.data(), dw0.size()}, {dw1.data(), dw1.size()}, {dw2.data(), dw2.size()}, {dw3.data(), dw3.size()}, {pdb[0], 16}, {pdb[1], 16}, {pdb[2], 16}, {pdb[3], 16}});
        if (mask & 1) continue;
        snprintf(what, sizeof(what), "wgrad_x3_dense_reduce db mask %d", mask >> 1);
        check(what, wgrad_x3_dense_reduce{{dw1.data(), dw2.data(), dw3.data()}, {pdb[1], pdb[2], pdb[3]}},
              {{dw1.data(), dw1.size()}, {dw2.data(), dw2.size()}, {dw3.data(), dw3.size()}, {pdb[1], 16}, {pdb[2], 16}, {pdb[3], 16}});
    }
    printf("%d map cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
