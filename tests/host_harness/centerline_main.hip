// tests/host_harness/centerline_main.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the centreline rule's per-word decisions (f1tenth_gym_amd/csrc/f110_math.hpp: cl_pass_word and what it
// calls), as a stand-alone program for tests/test_centerline_host.py: it packs a free mask into a bit plane exactly as the kernels
// hold it, runs the passes of steps 1 - 3 on the CPU between two planes, and writes the final mask and the three deletion totals.
//   centerline_main IN OUT    IN: int32 H, W, max_passes, then [H][W] bytes (1 free);  OUT: int64 deleted[3], int64 converged,
//                             then [H][W] bytes (1 set)
//   centerline_main           a self-check on rings of widths around the word size (also run under the host sanitizers)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

struct Plane {
    int H, W, Ww;
    std::vector<uint64_t> w;
    Plane(int H_, int W_) : H(H_), W(W_), Ww((W_ + 63) / 64), w((size_t)H_ * ((W_ + 63) / 64), 0) {}
    bool at(int r, int c) const { return (w[(size_t)r * Ww + (c >> 6)] >> (c & 63)) & 1u; }
    void set(int r, int c) { w[(size_t)r * Ww + (c >> 6)] |= 1ull << (c & 63); }
};

static long long one_pass(int op, const Plane &src, Plane &dst)
{
    long long n = 0;
    for (int r = 0; r < src.H; ++r)
        for (int w = 0; w < src.Ww; ++w) {
            uint64_t out;
            n += __builtin_popcountll(cl_pass_word(op, src.w.data(), src.H, src.Ww, r, w, out));
            dst.w[(size_t)r * src.Ww + w] = out;
        }
    return n;
}

// steps 1 - 3; false: not converged within max_passes
static bool skeleton(Plane &a, int max_passes, long long deleted[3])
{
    Plane b(a.H, a.W);
    deleted[0] = deleted[1] = deleted[2] = 0;
    for (int used = 0;; ++used) {
        if (used == max_passes) return false;
        const long long n = one_pass(0, a, b) + one_pass(1, b, a);
        deleted[0] += n;
        if (n == 0) break;
    }
    deleted[1] += one_pass(2, a, b);
    deleted[1] += one_pass(3, b, a);
    deleted[1] += one_pass(4, a, b);
    deleted[1] += one_pass(5, b, a);
    for (int used = 0;; ++used) {
        if (used == max_passes) return false;
        const long long n = one_pass(6, a, b);
        std::swap(a.w, b.w);
        deleted[2] += n;
        if (n == 0) break;
    }
    return true;
}

static int self_check()
{
    const int widths[] = {33, 63, 64, 65, 127, 128, 130};
    long long total = 0;
    for (int W : widths) {
        const int H = 40;
        Plane p(H, W);
        for (int r = 0; r < H; ++r)   // a ring that touches every border, three cells wide
            for (int c = 0; c < W; ++c)
                if (r < 3 || r >= H - 3 || c < 3 || c >= W - 3) p.set(r, c);
        long long d[3];
        if (!skeleton(p, 4 * (H + W), d)) {
            std::printf("width %d: not converged\n", W);
            return 1;
        }
        long long left = 0;
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                if (!p.at(r, c)) continue;
                ++left;
                int deg = 0;
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc)
                        if ((dr || dc) && r + dr >= 0 && r + dr < H && c + dc >= 0 && c + dc < W && p.at(r + dr, c + dc)) ++deg;
                if (deg != 2) {
                    std::printf("width %d: cell (%d, %d) has %d neighbours\n", W, r, c, deg);
                    return 1;
                }
            }
        for (size_t i = 0; i < p.w.size(); ++i)   // nothing beyond column W
            if ((int)(i % p.Ww) == p.Ww - 1 && (W & 63) && (p.w[i] >> (W & 63))) {
                std::printf("width %d: bits beyond the last column\n", W);
                return 1;
            }
        total += left;
    }
    std::printf("ok: %zu rings, %lld loop cells\n", sizeof widths / sizeof widths[0], total);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return self_check();
    std::FILE *f = std::fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1) return 2;
    const int H = hdr[0], W = hdr[1];
    std::vector<unsigned char> bytes((size_t)H * W);
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
    std::fclose(f);
    Plane p(H, W);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c)
            if (bytes[(size_t)r * W + c]) p.set(r, c);
    long long d[3];
    const int64_t ok = skeleton(p, hdr[2] > 0 ? hdr[2] : 4 * (H + W), d) ? 1 : 0;
    const int64_t head[4] = {d[0], d[1], d[2], ok};
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) bytes[(size_t)r * W + c] = p.at(r, c) ? 1 : 0;
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(head, sizeof head, 1, f) != 1 || std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
    std::fclose(f);
    return 0;
}
