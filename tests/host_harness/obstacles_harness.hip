// tests/host_harness/obstacles_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the obstacle stamp (f1tenth_gym_amd/csrc/f110_math.hpp: obstacle_hit, obstacle_cell_box), for
// tests/test_obstacles_host.py: the mask of a list of shapes, stamped over each shape's cell box exactly as k_obst_stamp does, is
// compared with the NumPy model bit for bit without a GPU.  Built with -DOBST_HARNESS_MAIN it is a stand-alone program (its own
// main) for a run under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// obs [n] (struct f110_obstacle's layout); mask [H][W] is zeroed here; boxes [n][4] = c0, c1, r0, r1 (or NULL).  whole_table != 0:
// the hit test runs over every cell instead of the cell box (what the box must not change).
void hh_obstacles_stamp(const Obstacle *obs, int n, int H, int W, double res, double ox, double oy, double oc, double os, int whole_table,
                        unsigned char *mask, int *boxes)
{
    const ObstFrame f{res, ox, oy, oc, os};
    std::memset(mask, 0, (size_t)H * W);
    for (int i = 0; i < n; ++i) {
        int c0, c1, r0, r1;
        obstacle_cell_box(obs[i], f, H, W, c0, c1, r0, r1);
        if (boxes) {
            boxes[4 * i + 0] = c0;
            boxes[4 * i + 1] = c1;
            boxes[4 * i + 2] = r0;
            boxes[4 * i + 3] = r1;
        }
        if (whole_table) {
            c0 = r0 = 0;
            c1 = W - 1;
            r1 = H - 1;
        }
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c)
                if (obstacle_hit(obs[i], f, r, c)) mask[(size_t)r * W + c] = 1;
    }
}

}

#ifdef OBST_HARNESS_MAIN
// boxes and discs inside, across every edge of, and far outside a 61 x 47 table (a rotated origin), extreme sizes included: the
// boxed stamp must equal the whole-table stamp, and no cell box may leave the table
int main()
{
    const int H = 61, W = 47;
    std::vector<Obstacle> obs;
    const double xs[] = {-1e300, -5.0, -0.3, 0.0, 0.4, 1.1, 2.3, 2.4, 9.0, 1e300};
    const double hs[] = {0.0, 0.02, 0.3, 4.0, 1e300};
    for (double x : xs)
        for (double y : xs)
            for (double hl : hs)
                for (int shape = 0; shape < 2; ++shape) obs.push_back(Obstacle{shape, 0, x, y, 0.8, 0.6, hl, 0.5 * hl});
    std::vector<unsigned char> a((size_t)H * W), b((size_t)H * W);
    std::vector<int> boxes(4 * obs.size());
    long stamped = 0;
    for (size_t i = 0; i < obs.size(); ++i) {
        hh_obstacles_stamp(&obs[i], 1, H, W, 0.05, -0.4, -0.2, 0.9800665778412416, 0.19866933079506122, 0, a.data(), &boxes[4 * i]);
        hh_obstacles_stamp(&obs[i], 1, H, W, 0.05, -0.4, -0.2, 0.9800665778412416, 0.19866933079506122, 1, b.data(), nullptr);
        if (std::memcmp(a.data(), b.data(), a.size()) != 0) {
            std::printf("obstacle %zu: the cell box drops stamped cells\n", i);
            return 1;
        }
        const int *q = &boxes[4 * i];
        if (q[0] < 0 || q[2] < 0 || q[1] > W - 1 || q[3] > H - 1) {
            std::printf("obstacle %zu: cell box [%d, %d] x [%d, %d] leaves the table\n", i, q[0], q[1], q[2], q[3]);
            return 1;
        }
        for (unsigned char v : a) stamped += v;
    }
    std::printf("ok: %zu obstacles, %ld stamped cells\n", obs.size(), stamped);
    return 0;
}
#endif
