// tests/host_harness/neighbors_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the neighbour arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, nbr_*), for
// tests/test_neighbors_host.py: eligibility, the sorted insertion, the channels, the gap's wrap, padding and scaling are compared
// with the Python model without a GPU.  The GPU tests hold the device instantiation (and the kernel around it) to the same model.
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// in [m][5] = x, y, theta, v, s, env-major, m a multiple of A; out [m][K][D], raw [m][K][10], idx [m][K].  L > 0 wraps the gap.
// The caller has validated the settings.
void hh_neighbors(int A, int K, int channels, double max_range, double pad, const double *scale, double L, const double *in, int m,
                  float *out, double *raw, int *idx)
{
    NbrSpec sp{};
    sp.K = K;
    sp.KT = 1;
    while (sp.KT < K) sp.KT *= 2;
    sp.channels = channels;
    sp.R2 = max_range * max_range;
    sp.pad = pad;
    for (int b = 0; b < NBR_NCHANNELS; ++b) {
        sp.scale[b] = scale[b];
        sp.D += channels >> b & 1;
    }
    std::vector<NbrAgent> env((size_t)A);
    for (int e = 0; e < m / A; ++e) {
        const size_t i = (size_t)e * A;
        const double *rows = in + 5 * i;
        float *o = out + i * K * sp.D;
        double *rw = raw + i * K * NBR_NCHANNELS;
        int32_t *ix = idx + i * K;
        switch (sp.KT) {
        case 1: nbr_env<1>(sp, rows, A, L, env.data(), o, rw, ix); break;
        case 2: nbr_env<2>(sp, rows, A, L, env.data(), o, rw, ix); break;
        case 4: nbr_env<4>(sp, rows, A, L, env.data(), o, rw, ix); break;
        default: nbr_env<8>(sp, rows, A, L, env.data(), o, rw, ix); break;
        }
    }
}

}
