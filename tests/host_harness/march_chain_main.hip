// tests/host_harness/march_chain_main.hip — TEST TOOLING, not part of the product.
//
// march_padded (f1tenth_gym_amd/csrc/f110_math.hpp) as a stand-alone HOST program for the address and undefined-behaviour
// sanitizers (tests/test_host_march_chain.py builds and runs it; nothing of it is loaded into Python).  The padded table is a
// heap block of exactly pad_width * pad_height doubles; every byte offset the loop forms is checked against its size by this
// program itself (F110_MARCH_OFFSET_HOOK), a load just past either end by the sanitizer's red zones as well, and the conversions
// that form the offset (double -> int, shifts, 24-bit products) by UBSan.
//
//   march_chain_main TABLE H W RES OX OY OYAW POSES N_POSES BEAMS FOV
// TABLE: H x W float64 distance table (row-major, raw), POSES: N_POSES x 3 float64 (x, y, theta), raw.
// Prints "ok: <rays> rays, fast <n> guard <n> far <n>, lookups <n>, offsets checked <n>, sum <range sum>".
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include <hip/hip_runtime.h>
#include <stdint.h>

// every byte offset march_padded is about to load from, against the table this program built: inside it and on a cell
static unsigned long long g_pad_bytes = 0, g_offsets_checked = 0;
static inline __host__ __device__ void check_march_offset(uint32_t off)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if ((unsigned long long)off + 8ull > g_pad_bytes || (off & 7u)) {
        fprintf(stderr, "march_padded formed byte offset %u for a table of %llu bytes\n", off, g_pad_bytes);
        abort();
    }
    ++g_offsets_checked;
#else
    (void)off;
#endif
}
#define F110_MARCH_OFFSET_HOOK(off) check_march_offset(off)
#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

static std::vector<double> read_doubles(const char *path, size_t n)
{
    std::vector<double> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(double), n, f) != n) {
        fprintf(stderr, "cannot read %zu doubles from %s\n", n, path);
        exit(2);
    }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 12) {
        fprintf(stderr, "usage: %s TABLE H W RES OX OY OYAW POSES N_POSES BEAMS FOV\n", argv[0]);
        return 2;
    }
    const int H = atoi(argv[2]), W = atoi(argv[3]);
    const double res = atof(argv[4]), ox = atof(argv[5]), oy = atof(argv[6]), oyaw = atof(argv[7]);
    const int n_poses = atoi(argv[9]), B = atoi(argv[10]);
    const double fov = atof(argv[11]);
    const std::vector<double> dt = read_doubles(argv[1], (size_t)H * W);
    const std::vector<double> poses = read_doubles(argv[8], (size_t)n_poses * 3);
    const int theta_dis = 2000;

    // the constants as tests/host_harness/harness.hip (hh_scan) and the library's finish_map() set them
    ScanConst k{};
    std::vector<double2> cs(theta_dis);
    for (int i = 0; i < theta_dis; ++i) {
        const double a = kTwoPi * (double)i / (double)(theta_dis - 1);
        cs[i] = make_double2(cos(a), sin(a));   // direction 0 is (1, 0) exactly: a beam along y = const
    }
    k.cs = cs.data();
    k.height = H; k.width = W; k.row_bytes = W * 8; k.theta_dis = theta_dis; k.num_beams = B;
    k.res = res; k.inv_res = 1.0 / res;
    int e; k.res_pow2 = (frexp(res, &e) == 0.5) ? 1 : 0;
    k.orig_x = ox; k.orig_y = oy; k.orig_c = cos(oyaw); k.orig_s = sin(oyaw);
    k.ident_rot = (k.orig_c == 1.0 && k.orig_s == 0.0) ? 1 : 0;
    k.w_res = W * res; k.h_res = H * res;
    k.oob_value = dt[(size_t)H * W - 1];
    k.eps = 1e-4; k.max_range = 30.0; k.fov = fov;
    k.theta_inc = theta_dis * (fov / (B - 1)) / (2. * kPi);
    const double g = 64.0 * (double)B * 2.2737367544323206e-13;
    k.dir_guard = g > 1e-8 ? g : 1e-8;
    k.inv_theta_dis = 1.0 / (double)theta_dis;
    k.table = dt.data();
    k.table_rm = dt.data();
    if (!setup_padded(k)) {
        fprintf(stderr, "the map does not fit the padded layout\n");
        return 2;
    }
    // exactly sized, on the heap: one element past either end is a red zone
    const size_t cells = (size_t)k.pad_width * k.pad_height;
    std::unique_ptr<double[]> padded(new double[cells]);
    for (size_t i = 0; i < cells; ++i) padded[i] = k.oob_value;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) padded[(size_t)(r + k.pad_border) * k.pad_width + (c + k.pad_border)] = dt[(size_t)r * W + c];
    k.pad = padded.get();
    g_pad_bytes = (unsigned long long)cells * 8ull;

    long long fast = 0, guard = 0, far = 0, lookups = 0, rays = 0;
    double sum = 0.0;
    for (int p = 0; p < n_poses; ++p) {
        const double x = poses[3 * p], y = poses[3 * p + 1], th = poses[3 * p + 2];
        const double start = scan_start_index(k, th);
        int hr, hc;
        const double d0 = k.ident_rot ? sample_distance<3, false, true>(k, nullptr, x, y, hr, hc)
                                      : sample_distance<3, false, false>(k, nullptr, x, y, hr, hc);
        double ux, uy;
        if (k.ident_rot) padded_position<true>(k, x, y, ux, uy);
        else padded_position<false>(k, x, y, ux, uy);
        if (!padded_start_ok(k, ux, uy)) {   // the kernels never enter march_padded from such a lidar
            far += B;
            rays += B;
            continue;
        }
        for (int b = 0; b < B; ++b) {
            const double2 d = cs[beam_dir_index(k, start, b)];
            double cux, cuy, r = 0.0;
            if (k.ident_rot) padded_rate<true>(k, d.x, d.y, cux, cuy);
            else padded_rate<false>(k, d.x, d.y, cux, cuy);
            int nl = 0;
            const bool ok = (b & 1) ? march_padded<true>(k, ux, uy, cux, cuy, d0, r, hr, hc, nl)
                                    : march_padded<false>(k, ux, uy, cux, cuy, d0, r, hr, hc, nl);
            if (ok) {
                ++fast;
                sum += r;
                lookups += nl;
                if ((b & 1) && nl > 1 && !((hr == -1 && hc == -1) || (hr >= 0 && hr < H && hc >= 0 && hc < W))) {
                    fprintf(stderr, "pose %d beam %d: hit cell (%d, %d) outside the map\n", p, b, hr, hc);
                    return 1;
                }
            } else {
                ++guard;
            }
            ++rays;
        }
    }
    printf("ok: %lld rays, fast %lld guard %lld far %lld, lookups %lld, offsets checked %llu, sum %.17g\n", rays, fast, guard, far, lookups,
           g_offsets_checked, sum);
    return 0;
}
