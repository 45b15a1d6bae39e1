// tests/host_harness/obs_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the observation encoder's per-row arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, obs_*), for
// tests/test_obs_encoder_host.py: sector bounds, pooling, clip / scale / cast, feature order and the frame rule are compared
// with the NumPy model without a GPU.  The GPU tests hold the device instantiation (and the kernel around it) to the same model.
#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// scans [m][B], cols [m][8] (feature sources in bit order), step_count [m], inout [m][F][D]; feat_scale [8] indexed by bit.
// Returns D (the caller has validated the settings: this is the arithmetic only).
int hh_obs_encode(int beam_lo, int beam_hi, int K, int pool, int features, const double *feat_scale, double clip, double scale, int F,
                  int fill, const double *scans, int B, const double *cols, const int *step_count, int m, float *inout)
{
    ObsRowSpec s{};
    s.W = beam_hi - beam_lo;
    s.K = K;
    s.pool = pool;
    s.clip = clip;
    s.scale = scale;
    for (int c = 0; c < kObsFeatures; ++c) {
        if (!(features >> c & 1)) continue;
        s.feat[s.nfeat] = c;
        s.feat_scale[s.nfeat++] = feat_scale[c];
    }
    s.D = K + s.nfeat;
    for (int i = 0; i < m; ++i)
        obs_update_stack(s, scans + (size_t)i * B + beam_lo, cols + (size_t)i * kObsFeatures, 1, step_count[i], fill, F,
                         inout + (size_t)i * F * s.D);
    return s.D;
}

}
