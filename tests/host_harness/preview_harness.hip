// tests/host_harness/preview_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the track preview's per-station arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, preview_*), for
// tests/test_track_preview_host.py: station arc length, segment search, interpolation, frame and scaling are compared with the
// NumPy model without a GPU.  The GPU tests hold the device instantiation (and the kernel around it) to the same model.
#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// cols [7][nseg] (ax, ay, dx, dy, l2, len, cum), attr [C][npts] or null, in [m][4] = x, y, theta, s; out [m][P][D], raw [m][P][8],
// seg [m][P].  The caller has validated the settings.
void hh_track_preview(const double *cols, int nseg, int closed, double L, const double *attr, int C, int npts, int P, int channels,
                      int frame, double offset, double spacing, const double *scale, const double *in, int m, float *out, double *raw,
                      int *seg)
{
    PreviewSpec sp{};
    sp.P = P;
    sp.channels = channels;
    sp.frame = frame;
    sp.offset = offset;
    sp.spacing = spacing;
    for (int b = 0; b < PREVIEW_NCHANNELS; ++b) {
        sp.scale[b] = scale[b];
        sp.D += channels >> b & 1;
    }
    PreviewTrack tr{};
    tr.cols = cols;
    tr.attr = attr;
    tr.nseg = nseg;
    tr.closed = closed;
    tr.C = C;
    tr.npts = npts;
    tr.L = L;
    for (int i = 0; i < m; ++i) {
        const double *r = in + 4 * (size_t)i;
        preview_row(sp, tr, r[0], r[1], r[2], r[3], out + (size_t)i * P * sp.D, raw + (size_t)i * P * PREVIEW_NCHANNELS, seg + (size_t)i * P);
    }
}

}
