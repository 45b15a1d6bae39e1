// tests/host_harness/corridor_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the corridor carve's mask (f1tenth_gym_amd/csrc/f110_math.hpp: cell_centre, corridor_seg, corridor_hit,
// corridor_tile, corridor_reaches, corridor_list_slot), for tests/test_trackgen_host.py: the same per-cell decision AND the same
// tile-and-cull walk as k_corridor_mask — tiles of kCorrTileH x kCorrTileW cells, the segment list walked kCorrChunk at a time, a
// kept list of kCorrCap entries that is swept when it is full — in plain loops, so that the mask, the carved count and the largest
// per-tile kept count can be compared with the NumPy model without a GPU.  Built with -DCORR_HARNESS_MAIN it is a stand-alone
// program (its own main) for a run under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// out [4] = kCorrTileH, kCorrTileW, kCorrChunk, kCorrCap as built
void hh_corridor_consts(int *out)
{
    out[0] = kCorrTileH;
    out[1] = kCorrTileW;
    out[2] = kCorrChunk;
    out[3] = kCorrCap;
}

// xy [M][2], hw [S]; mask [H][W] (every cell is written), *carved the number of ones, *max_kept the largest number of segments a
// tile kept, *rounds how often a full list was swept, *cell_tests the calls of corridor_hit.  cull == 0: every tile keeps every
// segment (what culling must not change).
void hh_corridor_mask(const double *xy, const double *hw, int M, int closed, int H, int W, double res, double ox, double oy, double oc, double os, int cull,
                      unsigned char *mask, long long *carved, int *max_kept, long long *rounds, long long *cell_tests)
{
    const ObstFrame f{res, ox, oy, oc, os};
    const int S = closed ? M : M - 1;
    std::vector<CorridorSeg> list((size_t)kCorrCap);
    *carved = 0;
    *max_kept = 0;
    *rounds = 0;
    *cell_tests = 0;
    for (int r0 = 0; r0 < H; r0 += kCorrTileH)
        for (int c0 = 0; c0 < W; c0 += kCorrTileW) {
            const int c1 = (c0 + kCorrTileW < W ? c0 + kCorrTileW : W) - 1, r1 = (r0 + kCorrTileH < H ? r0 + kCorrTileH : H) - 1;
            const CorridorTile tile = corridor_tile(f, r0, c0, r1, c1);
            for (int r = r0; r <= r1; ++r)
                for (int c = c0; c <= c1; ++c) mask[(size_t)r * W + c] = 0;
            // a sweep: every cell of the tile inside the ring that is not carved yet, against the list, leaving at the first hit
            const auto sweep = [&](int count) {
                for (int r = r0; r <= r1; ++r)
                    for (int c = c0; c <= c1; ++c) {
                        if (!(r > 0 && r < H - 1 && c > 0 && c < W - 1) || mask[(size_t)r * W + c]) continue;
                        double wx, wy;
                        cell_centre(f, r, c, wx, wy);
                        for (int i = 0; i < count; ++i) {
                            ++*cell_tests;
                            if (corridor_hit(list[(size_t)i], wx, wy)) {
                                mask[(size_t)r * W + c] = 1;
                                break;
                            }
                        }
                    }
            };
            int n = 0, kept_here = 0;
            for (int s0 = 0; s0 < S; s0 += kCorrChunk) {
                const int end = s0 + kCorrChunk < S ? s0 + kCorrChunk : S;
                std::vector<int> keep;   // the chunk's kept segments, in segment order
                for (int s = s0; s < end; ++s) {
                    const int e = s + 1 == M ? 0 : s + 1;
                    if (!cull || corridor_reaches(xy[2 * s], xy[2 * s + 1], xy[2 * e], xy[2 * e + 1], hw[s], tile)) keep.push_back(s);
                }
                const int total = (int)keep.size();
                kept_here += total;
                const auto put = [&](bool first) {
                    for (int j = 0; j < total; ++j) {
                        const int slot = corridor_list_slot(n + j, first);
                        if (slot < 0) continue;
                        const int s = keep[(size_t)j], e = s + 1 == M ? 0 : s + 1;
                        list.at((size_t)slot) = corridor_seg(xy[2 * s], xy[2 * s + 1], xy[2 * e], xy[2 * e + 1], hw[s]);
                    }
                };
                put(true);
                if (n + total > kCorrCap) {
                    sweep(kCorrCap);
                    ++*rounds;
                    put(false);
                    n += total - kCorrCap;
                } else {
                    n += total;
                }
            }
            sweep(n);
            if (kept_here > *max_kept) *max_kept = kept_here;
            for (int r = r0; r <= r1; ++r)
                for (int c = c0; c <= c1; ++c) *carved += mask[(size_t)r * W + c];
        }
}

}

#ifdef CORR_HARNESS_MAIN
// Lines inside, across every edge of, and far outside a 45 x 130 table under a turned origin that is no rotation, extreme sizes
// included, and a wound line that overflows the kept list: the culled walk must equal the walk that keeps every segment, cell for
// cell, and the ring must stay 0.
static int check(const char *what, const std::vector<double> &xy, const std::vector<double> &hw, int closed, int H, int W, long long *total)
{
    const int M = (int)(xy.size() / 2);
    std::vector<unsigned char> a((size_t)H * W, 7), b((size_t)H * W, 7);
    long long ca, cb, ra, rb, ta, tb;
    int ka, kb;
    hh_corridor_mask(xy.data(), hw.data(), M, closed, H, W, 0.05, -0.4, -0.2, 0.97, 0.21, 1, a.data(), &ca, &ka, &ra, &ta);
    hh_corridor_mask(xy.data(), hw.data(), M, closed, H, W, 0.05, -0.4, -0.2, 0.97, 0.21, 0, b.data(), &cb, &kb, &rb, &tb);
    if (std::memcmp(a.data(), b.data(), a.size()) != 0 || ca != cb) {
        std::printf("%s: culling changes the mask (%lld against %lld carved)\n", what, ca, cb);
        return 1;
    }
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c)
            if ((r == 0 || r == H - 1 || c == 0 || c == W - 1) && a[(size_t)r * W + c]) {
                std::printf("%s: ring cell (%d, %d) is carved\n", what, r, c);
                return 1;
            }
    *total += ca;
    return 0;
}

int main()
{
    const int H = 45, W = 130;
    long long total = 0;
    const double xs[] = {-1e300, -1e160, -7.0, -0.3, 0.0, 0.4, 1.1, 2.3, 5.9, 40.0, 1e160, 1e300};
    const double hs[] = {0.0, 0.02, 0.3, 4.0, 1e160, 1e300};
    int n = 0;
    for (double x0 : xs)
        for (double y0 : xs)
            for (double hw : hs) {
                const std::vector<double> open{x0, y0, 1.7, 0.9, 1.7, 0.9, 3.1, y0}, closed{x0, y0, 1.7, 0.9, 3.1, 1.4};
                if (check("open", open, std::vector<double>{hw, 0.5 * hw, 0.1}, 0, H, W, &total)) return 1;
                if (check("closed", closed, std::vector<double>{hw, 0.1, 0.5 * hw}, 1, H, W, &total)) return 1;
                n += 2;
            }
    // 2 * kCorrCap + 3 points wound inside one tile, and one more than the list holds
    for (int M : {kCorrCap - 1, kCorrCap, kCorrCap + 1, 2 * kCorrCap + 3}) {
        std::vector<double> xy, hw;
        for (int i = 0; i < M; ++i) {
            const int row = i / 8, k = i % 8;
            xy.push_back(3.3 + 0.31 * (row % 2 ? 7 - k : k));
            xy.push_back(1.05 + 0.0009 * row);
        }
        hw.assign((size_t)M - 1, 0.0721);
        std::vector<unsigned char> a((size_t)H * W);
        long long c, r, t;
        int kept;
        hh_corridor_mask(xy.data(), hw.data(), M, 0, H, W, 0.05, -0.4, -0.2, 0.97, 0.21, 1, a.data(), &c, &kept, &r, &t);
        if (M == 2 * kCorrCap + 3 && (kept <= kCorrCap || r < 1)) {
            std::printf("the wound line does not overflow the list: %d kept, %lld rounds\n", kept, r);
            return 1;
        }
        if (check("wound", xy, hw, 0, H, W, &total)) return 1;
        ++n;
    }
    std::printf("ok: %d lines, %lld carved cells\n", n, total);
    return 0;
}
#endif
