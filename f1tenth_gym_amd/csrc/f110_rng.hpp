// f110_rng.hpp — the scan-noise stream of the reference, generated on the device.
//
// The reference adds `rng.normal(0., 0.01, size=num_beams)` to every scan (laser_models.py:450-452)
// with `rng = np.random.default_rng(seed=self.seed)` re-created at every reset
// (base_classes.py:204), i.e. NumPy's PCG64 bit generator (128-bit LCG, XSL-RR output) feeding
// NumPy's 256-layer ziggurat `random_standard_normal` (numpy/random/src/distributions/
// distributions.c; third-party dependency of the reference, pinned `numpy>=1.18,<=1.22` in its
// setup.py, present here as 2.2.6 — the algorithm and its constants are unchanged across those
// versions).  This header restates that algorithm so that the device produces the SAME doubles:
//
//   pcg_step / pcg_output      pcg64.h: state = state * MULT + inc; out = rotr64(hi ^ lo, hi >> 58)
//   pcg64_seed_from_u64        SeedSequence(entropy).generate_state(4, uint64) + pcg64_set_seed
//   zig_attempt                one pass of random_standard_normal's for(;;) body for the draw at a
//                              given stream position: accept (1 draw), wedge test (2 draws, may
//                              reject), tail loop (1 + 2k draws)
//   zig_chain_starts           which positions of a 64-draw chunk start an attempt, given how many
//                              draws every attempt consumes — the only sequential dependency of the
//                              stream, resolved with a few scalar iterations per chunk
//   log1p_glibc                glibc 2.35's log1p (the tail's output value goes through it, so it
//                              must match to the bit; checked on 5*10^7 arguments)
//
// Everything is __host__ __device__ so tests/host_harness runs the same code on the CPU against
// NumPy's live stream.  The wedge test compares against exp(); device and glibc exp may differ by
// an ulp, which can flip the comparison only when both sides agree to ~2^-52 relative (about one
// wedge test in 10^15) — accepted like the other measure-zero deviations listed in DESIGN.md.
#pragma once

#include <stdio.h>

#include "f110_math.hpp"
#include "f110_ziggurat_tables.hpp"

namespace f110 {

struct U128 {
    uint64_t hi, lo;
};

F110_HD uint64_t mulhi_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

F110_HD U128 mul128(U128 a, U128 b)
{
    U128 r;
    r.lo = a.lo * b.lo;
    r.hi = mulhi_u64(a.lo, b.lo) + a.hi * b.lo + a.lo * b.hi;
    return r;
}

F110_HD U128 add128(U128 a, U128 b)
{
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}

// PCG_DEFAULT_MULTIPLIER_128 (pcg64.h)
constexpr uint64_t kPcgMultHi = 2549297995355413924ULL, kPcgMultLo = 4865540595714422341ULL;

F110_HD U128 pcg_step(U128 s, U128 inc)
{
    const U128 m = {kPcgMultHi, kPcgMultLo};
    return add128(mul128(s, m), inc);
}

// pcg_output_xsl_rr_128_64 of the state AFTER the step (pcg64_next64 steps first)
F110_HD uint64_t pcg_output(U128 s)
{
    const uint64_t x = s.hi ^ s.lo;
    const unsigned rot = (unsigned)(s.hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// next_double: (next_uint64 >> 11) * 2^-53
F110_HD double pcg_to_double(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// Jump constants: the state i steps ahead is A^i * s + G_i * inc with G_i = 1 + A + ... + A^(i-1)
// (both independent of the seed), i = 0..64.
struct PcgJump {
    U128 a[65], g[65];
};

inline void pcg_jump_table(PcgJump &t)
{
    const U128 m = {kPcgMultHi, kPcgMultLo};
    t.a[0] = {0, 1};
    t.g[0] = {0, 0};
    for (int i = 1; i <= 64; ++i) {
        t.a[i] = mul128(t.a[i - 1], m);
        t.g[i] = add128(mul128(t.g[i - 1], m), U128{0, 1});
    }
}

// np.random.SeedSequence(seed).generate_state(4, np.uint64) -> pcg64_set_seed: out = {state.hi,
// state.lo, inc.hi, inc.lo} of np.random.PCG64(seed) (numpy/random/bit_generator.pyx,
// _pcg64.pyx, src/pcg64/pcg64.h).  seed is a non-negative integer below 2^64.
inline void pcg64_seed_from_u64(uint64_t seed, uint64_t out[4])
{
    const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
    const uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    uint32_t entropy[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int n_ent = (seed >> 32) ? 2 : 1;
    uint32_t pool[4], hc = INIT_A;
    auto hashmix = [&](uint32_t v) {
        v ^= hc;
        hc *= MULT_A;
        v *= hc;
        v ^= v >> 16;
        return v;
    };
    auto mix = [&](uint32_t x, uint32_t y) {
        uint32_t r = MIX_L * x - MIX_R * y;
        r ^= r >> 16;
        return r;
    };
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < n_ent ? entropy[i] : 0u);
    for (int s = 0; s < 4; ++s)
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    uint32_t w[8], hb = INIT_B;
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3];
        v ^= hb;
        hb *= MULT_B;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    uint64_t q[4];
    for (int i = 0; i < 4; ++i) q[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    // pcg64_set_seed: initstate = (q0 << 64) | q1, initseq = (q2 << 64) | q3; pcg_setseq_128_srandom_r
    const U128 initstate = {q[0], q[1]}, initseq = {q[2], q[3]};
    U128 inc = {(initseq.hi << 1) | (initseq.lo >> 63), (initseq.lo << 1) | 1ull};
    U128 st = {0, 0};
    st = pcg_step(st, inc);
    st = add128(st, initstate);
    st = pcg_step(st, inc);
    out[0] = st.hi;
    out[1] = st.lo;
    out[2] = inc.hi;
    out[3] = inc.lo;
}

// np.random.PCG64(np.random.SeedSequence(entropy, spawn_key=(e,))) = SeedSequence(entropy).spawn(E)[e]: the same words as above
// for the assembled entropy — the run entropy as little-endian uint32 words (NumPy's _coerce_to_uint32_array of the seed),
// zero-filled to the pool size because a spawn key follows, then the words of e (0 -> [0]).  Words past the pool size are mixed
// into every pool word after the pool's own cross-mix (bit_generator.pyx mix_entropy).
inline void pcg64_seed_spawn(const uint32_t *run, int n_run, uint64_t e, uint64_t out[4])
{
    const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
    const uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    const uint32_t key[2] = {(uint32_t)e, (uint32_t)(e >> 32)};
    const int n_key = (e >> 32) ? 2 : 1;
    const int n_pre = n_run > 4 ? n_run : 4, n_all = n_pre + n_key;
    auto word = [&](int q) -> uint32_t { return q < n_pre ? (q < n_run ? run[q] : 0u) : key[q - n_pre]; };
    uint32_t pool[4], hc = INIT_A;
    auto hashmix = [&](uint32_t v) {
        v ^= hc;
        hc *= MULT_A;
        v *= hc;
        v ^= v >> 16;
        return v;
    };
    auto mix = [&](uint32_t x, uint32_t y) {
        uint32_t r = MIX_L * x - MIX_R * y;
        r ^= r >> 16;
        return r;
    };
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(word(i));
    for (int s = 0; s < 4; ++s)
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    for (int s = 4; s < n_all; ++s)
        for (int d = 0; d < 4; ++d) pool[d] = mix(pool[d], hashmix(word(s)));
    uint32_t w[8], hb = INIT_B;
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3];
        v ^= hb;
        hb *= MULT_B;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    uint64_t q[4];
    for (int i = 0; i < 4; ++i) q[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    const U128 initstate = {q[0], q[1]}, initseq = {q[2], q[3]};
    U128 inc = {(initseq.hi << 1) | (initseq.lo >> 63), (initseq.lo << 1) | 1ull};
    U128 st = {0, 0};
    st = pcg_step(st, inc);
    st = add128(st, initstate);
    st = pcg_step(st, inc);
    out[0] = st.hi;
    out[1] = st.lo;
    out[2] = inc.hi;
    out[3] = inc.lo;
}

// ---- glibc 2.35 log1p (sysdeps/ieee754/dbl-64/s_log1p.c: fdlibm's algorithm with the
// polynomial evaluated in the split form glibc uses), restated for x in (-1, 0] — the only
// arguments the ziggurat tail feeds it (-next_double).
F110_HD int32_t high_word(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2hiint(x);
#else
    uint64_t u;
    memcpy(&u, &x, 8);
    return (int32_t)(u >> 32);
#endif
}

F110_HD double with_high_word(double x, int32_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hiloint2double(h, __double2loint(x));
#else
    uint64_t u;
    memcpy(&u, &x, 8);
    u = (u & 0xffffffffull) | ((uint64_t)(uint32_t)h << 32);
    memcpy(&x, &u, 8);
    return x;
#endif
}

F110_HD double log1p_glibc(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double two54 = 1.80143985094819840000e+16;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    double f = 0., c = 0., u;
    int32_t hx = high_word(x), hu = 0, k = 1;
    const int32_t ax = hx & 0x7fffffff;
    if (hx < 0x3FDA827A) {  // x < 0.41422
        if (ax >= 0x3ff00000) return (x == -1.0) ? -HUGE_VAL : (x - x) / (x - x);
        if (ax < 0x3e200000) {  // |x| < 2^-29
            if (two54 + x > 0.0 && ax < 0x3c900000) return x;
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int32_t)0xbfd2bec3) {  // -0.2929 < x < 0.41422
            k = 0;
            f = x;
            hu = 1;
        }
    }
    if (k != 0) {
        u = 1.0 + x;
        hu = high_word(u);
        k = (hu >> 20) - 1023;
        c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);
        c /= u;
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = with_high_word(u, hu | 0x3ff00000);
        } else {
            k += 1;
            u = with_high_word(u, hu | 0x3fe00000);
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    if (hu == 0) {  // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return k * ln2_hi - ((R - (k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f), z = s * s;
    const double R1 = z * Lp1, z2 = z * z, R2 = Lp2 + z * Lp3, z4 = z2 * z2, R3 = Lp4 + z * Lp5, z6 = z4 * z2,
                 R4 = Lp6 + z * Lp7;
    const double R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return k * ln2_hi - ((hfsq - (s * (hfsq + R) + (k * ln2_lo + c))) - f);
}

// ---- ziggurat -------------------------------------------------------------------------------
constexpr double kZigR = 3.6541528853610087963519472518;       // ziggurat_nor_r
constexpr double kZigInvR = 0.27366123732975827203338247596;   // ziggurat_nor_inv_r

struct ZigTables {
    const uint64_t *k;  // ki_double
    const double *w;    // wi_double
    const double *f;    // fi_double
};

struct ZigAttempt {
    double val;  // the standard normal this attempt returns (when emit)
    int len;     // draws consumed, this one included
    bool emit;   // false: wedge test failed, random_standard_normal loops and the next attempt starts len draws on
};

// One pass of random_standard_normal's for(;;) body (distributions.c) for draw `r`; `st` is the
// generator state that produced r (further draws step from it).
F110_HD ZigAttempt zig_attempt(uint64_t r, U128 st, U128 inc, const ZigTables &t)
{
    ZigAttempt o;
    o.len = 1;
    o.emit = true;
    const int idx = (int)(r & 0xff);
    r >>= 8;
    const int sign = (int)(r & 0x1);
    const uint64_t rabs = (r >> 1) & 0x000fffffffffffffULL;
    double x = (double)rabs * t.w[idx];
    if (sign & 0x1) x = -x;
    o.val = x;
    if (rabs < t.k[idx]) return o;  // 99.3 % of the time
    if (idx == 0) {
        for (;;) {
            st = pcg_step(st, inc);
            const double u1 = pcg_to_double(pcg_output(st));
            st = pcg_step(st, inc);
            const double u2 = pcg_to_double(pcg_output(st));
            o.len += 2;
            const double xx = -kZigInvR * log1p_glibc(-u1);
            const double yy = -log1p_glibc(-u2);
            if (yy + yy > xx * xx) {
                o.val = ((rabs >> 8) & 0x1) ? -(kZigR + xx) : kZigR + xx;
                return o;
            }
        }
    }
    st = pcg_step(st, inc);
    const double u = pcg_to_double(pcg_output(st));
    o.len = 2;
    o.emit = ((t.f[idx - 1] - t.f[idx]) * u + t.f[idx]) < exp(-0.5 * x * x);
    return o;
}

F110_HD int ctz_u64(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__ffsll((unsigned long long)m) - 1;
#else
    return __builtin_ctzll(m);
#endif
}

F110_HD int popc_u64(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__popcll((unsigned long long)m);
#else
    return __builtin_popcountll(m);
#endif
}

// Positions (bits) of a 64-draw chunk at which an attempt starts.  `multi`: positions whose
// attempt — were one to start there — consumes more than one draw; len_of(p) its length;
// skip_in: leading positions already consumed by an attempt of the previous chunk; skip_out: the
// same for the next chunk.
template <typename LenOf>
F110_HD uint64_t zig_chain_starts(uint64_t multi, int skip_in, LenOf len_of, int &skip_out)
{
    if (skip_in >= 64) {
        skip_out = skip_in - 64;
        return 0ull;
    }
    uint64_t starts = ~0ull << skip_in;
    skip_out = 0;
    uint64_t m = multi & starts;
    while (m) {
        const int p = ctz_u64(m);
        m &= m - 1;
        const int last = p + len_of(p) - 1;  // the attempt at p consumes p .. last
        const uint64_t upto = last >= 63 ? ~0ull : ((1ull << (last + 1)) - 1ull);
        const uint64_t kill = upto & ~((2ull << p) - 1ull);  // p+1 .. min(last, 63)
        starts &= ~kill;
        m &= ~kill;
        if (last >= 64) skip_out = last - 63;
    }
    return starts;
}

// position of the (n+1)-th set bit of m (n < popcount(m))
F110_HD int nth_set_bit(uint64_t m, int n)
{
    for (int i = 0; i < n; ++i) m &= m - 1;
    return ctz_u64(m);
}

// the state n steps ahead, given (A_n, G_n): A_n * s + G_n * inc
F110_HD U128 pcg_jump(U128 s, U128 inc, U128 a, U128 g) { return add128(mul128(a, s), mul128(g, inc)); }

// the state `n` steps ahead
F110_HD U128 pcg_advance(U128 s, U128 inc, const U128 *ja, const U128 *jg, int n)
{
    while (n > 64) {
        s = pcg_jump(s, inc, ja[64], jg[64]);
        n -= 64;
    }
    return pcg_jump(s, inc, ja[n], jg[n]);
}

// ---- the MPPI planner's draws (include/f110.h, f110_mppi) ----------------------------------------------------------------------
// Generator.standard_normal() one draw after the other from one generator: what a candidate's lane does 2 H times
F110_HD double mppi_normal(U128 &st, U128 inc, const ZigTables &t)
{
    for (;;) {
        st = pcg_step(st, inc);
        const ZigAttempt z = zig_attempt(pcg_output(st), st, inc, t);
        for (int q = 1; q < z.len; ++q) st = pcg_step(st, inc);
        if (z.emit) return z.val;
    }
}

// PCG64.advance(n) for n = j * 2^kMppiJumpLog2, j = 0 .. 256, as (A_n, G_n): the state n steps ahead is A_n * s + G_n * inc
constexpr int kMppiJumpLog2 = 20;
constexpr int kMppiJumps = 257;   // entry 256 = 2^28 steps: where a call leaves the agent's generator

// (A_n, G_n) for n = j * 2^log2, j = 0 .. count - 1
inline void pcg_jump_table(U128 *a, U128 *g, int log2, int count)
{
    U128 a1 = {kPcgMultHi, kPcgMultLo}, g1 = {0, 1};
    for (int q = 0; q < log2; ++q) {            // A_2n = A_n * A_n, G_2n = G_n * (A_n + 1)
        g1 = mul128(g1, add128(a1, U128{0, 1}));
        a1 = mul128(a1, a1);
    }
    a[0] = {0, 1};
    g[0] = {0, 0};
    for (int j = 1; j < count; ++j) {           // A_(n+J) = A_n * A_J, G_(n+J) = G_n * A_J + G_J
        a[j] = mul128(a[j - 1], a1);
        g[j] = add128(mul128(g[j - 1], a1), g1);
    }
}

inline void mppi_jump_table(U128 *a, U128 *g) { pcg_jump_table(a, g, kMppiJumpLog2, kMppiJumps); }

// candidate k's row V[k][H][2] around the nominal U (fresh: (0, v_init)); stream = the agent's {state.hi, state.lo, inc.hi, inc.lo},
// (ja, jg) = entry k of the jump table.  Candidate 0 is the nominal itself, without a draw.
F110_HD void mppi_sample_row(const MppiSpec &s, const double *U, bool fresh, int k, const uint64_t *stream, U128 ja, U128 jg, const ZigTables &t,
                             double *row)
{
    if (k == 0) {
        for (int q = 0; q < 2 * s.H; ++q) row[q] = mppi_nominal(s, U, fresh, q >> 1, q & 1);
        return;
    }
    const U128 inc = {stream[2], stream[3]};
    U128 st = pcg_jump(U128{stream[0], stream[1]}, inc, ja, jg);
    for (int h = 0; h < s.H; ++h) {
        const double e_s = mppi_normal(st, inc, t);
        const double e_v = mppi_normal(st, inc, t);
        mppi_perturb(s, mppi_nominal(s, U, fresh, h, 0), mppi_nominal(s, U, fresh, h, 1), e_s, e_v, row + 2 * h);
    }
}

// ---- the particle filter's draws (include/f110.h, f110_pf) --------------------------------------------------------------------------
// Sub-stream q of an agent's generator is the generator advanced by q * 2^kPfJumpLog2 steps: entry q of the table, q = 0 .. P.  A
// call leaves the generator 2^28 steps on: entry kPfJumps - 1 (2^26 steps) four times.
constexpr int kPfJumpLog2 = 16;
constexpr int kPfJumps = 1025;

inline void pf_jump_table(U128 *a, U128 *g) { pcg_jump_table(a, g, kPfJumpLog2, kPfJumps); }

// sub-stream 0: Generator.random(), one output
F110_HD double pf_uniform(const uint64_t *stream)
{
    const U128 st = pcg_step(U128{stream[0], stream[1]}, U128{stream[2], stream[3]});
    return pcg_to_double(pcg_output(st));
}

// sub-stream p + 1 ((ja, jg) = entry p + 1): particle p's e_x, e_y, e_t
F110_HD void pf_normals(const uint64_t *stream, U128 ja, U128 jg, const ZigTables &t, double *e)
{
    const U128 inc = {stream[2], stream[3]};
    U128 st = pcg_jump(U128{stream[0], stream[1]}, inc, ja, jg);
    for (int q = 0; q < 3; ++q) e[q] = mppi_normal(st, inc, t);
}

// where a call leaves the generator; (ja, jg) = the table's last entry
F110_HD void pf_stream_advance(uint64_t *stream, U128 ja, U128 jg)
{
    const U128 inc = {stream[2], stream[3]};
    U128 st = {stream[0], stream[1]};
    for (int q = 0; q < 4; ++q) st = pcg_jump(st, inc, ja, jg);
    stream[0] = st.hi;
    stream[1] = st.lo;
}

// ---- the parameter sampler's draws (include/f110.h, f110_param_dist) -----------------------------------------------------------
// the layout of f110_param_dist
struct ParamDist {
    int32_t kind, scope;
    double a, b, lo, hi;
    int32_t relative, pad;
};
enum { kParamFixed = 0, kParamUniform = 1, kParamNormal = 2 };
enum { kParamScopeAgent = 0, kParamScopeEnv = 1 };

// one value of a drawn slot: Generator.uniform(a, b), or np.clip(Generator.normal(a, b), lo, hi)
F110_HD double param_draw_value(const ParamDist &d, U128 &st, U128 inc, const ZigTables &t)
{
    if (d.kind == kParamUniform) {
        st = pcg_step(st, inc);
        return d.a + pcg_to_double(pcg_output(st)) * (d.b - d.a);
    }
    const double v = d.a + d.b * mppi_normal(st, inc, t);
    return v < d.lo ? d.lo : (v > d.hi ? d.hi : v);
}

// one env's draw: slots in index order, within a slot the env's single value or agents 0 .. A - 1; only drawn slots of the env's
// rows [A][18] are written.  nominal [A][18] is read for relative slots only.
F110_HD void param_draw_env(const ParamDist *d, const double *nominal, int A, U128 &st, U128 inc, const ZigTables &t, double *rows)
{
    for (int p = 0; p < NPARAMS; ++p) {
        const ParamDist dp = d[p];
        if (dp.kind == kParamFixed) continue;
        double v = 0.0;
        if (dp.scope == kParamScopeEnv) v = param_draw_value(dp, st, inc, t);
        for (int s = 0; s < A; ++s) {
            if (dp.scope != kParamScopeEnv) v = param_draw_value(dp, st, inc, t);
            rows[(size_t)s * NPARAMS + p] = dp.relative ? nominal[(size_t)s * NPARAMS + p] * v : v;
        }
    }
}

// May these 18 entries be armed over the nominal rows [A][18]?  nullptr when they may, else the reason (in `msg`), which names the
// parameter.  Host only: validity is settled here, by intervals, so the draw has no rejection loop.
inline const char *param_dists_check(const ParamDist *d, const double *nominal, int A, char *msg, size_t cap)
{
    static const char *const name[NPARAMS] = {"mu", "C_Sf", "C_Sr", "lf", "lr", "h", "m", "I", "s_min", "s_max", "sv_min", "sv_max",
                                              "v_switch", "a_max", "v_min", "v_max", "width", "length"};
    auto fin = [](double v) { return v == v && v - v == 0.0; };
    double lo[NPARAMS], hi[NPARAMS];   // the interval v is drawn from (FIXED: unused)
    for (int p = 0; p < NPARAMS; ++p) {
        const ParamDist &e = d[p];
        if (e.kind < kParamFixed || e.kind > kParamNormal) return snprintf(msg, cap, "parameter %s: unknown kind %d", name[p], e.kind), msg;
        if (e.scope != kParamScopeAgent && e.scope != kParamScopeEnv) return snprintf(msg, cap, "parameter %s: unknown scope %d", name[p], e.scope), msg;
        if (e.kind == kParamFixed) continue;
        if (p == P_WIDTH || p == P_LENGTH)
            return snprintf(msg, cap, "parameter %s cannot be drawn: the collision boxes and the iTTC side tables are the constructor's", name[p]), msg;
        if (!fin(e.a) || !fin(e.b)) return snprintf(msg, cap, "parameter %s: a = %g, b = %g must be finite", name[p], e.a, e.b), msg;
        if (e.kind == kParamUniform) {
            if (e.a > e.b) return snprintf(msg, cap, "parameter %s: uniform needs a <= b, got %g, %g", name[p], e.a, e.b), msg;
            lo[p] = e.a;
            hi[p] = e.b;
        } else {
            if (e.b < 0.0) return snprintf(msg, cap, "parameter %s: normal needs scale >= 0, got %g", name[p], e.b), msg;
            if (!fin(e.lo) || !fin(e.hi)) return snprintf(msg, cap, "parameter %s: normal needs finite clip bounds, got %g, %g", name[p], e.lo, e.hi), msg;
            if (e.lo > e.hi) return snprintf(msg, cap, "parameter %s: normal needs lo <= hi, got %g, %g", name[p], e.lo, e.hi), msg;
            lo[p] = e.lo;
            hi[p] = e.hi;
        }
    }
    static const int positive[] = {P_MU, P_CSF, P_CSR, P_LF, P_LR, P_H, P_M, P_I, P_VSWITCH, P_AMAX};
    static const int below[][2] = {{P_SMIN, P_SMAX}, {P_SVMIN, P_SVMAX}, {P_VMIN, P_VMAX}};
    for (int s = 0; s < A; ++s) {
        const double *nom = nominal + (size_t)s * NPARAMS;
        double rl[NPARAMS], rh[NPARAMS];   // what the row of agent slot s can hold
        for (int p = 0; p < NPARAMS; ++p) {
            if (d[p].kind == kParamFixed) {
                rl[p] = rh[p] = nom[p];
                continue;
            }
            const double x = d[p].relative ? nom[p] * lo[p] : lo[p], y = d[p].relative ? nom[p] * hi[p] : hi[p];
            rl[p] = x < y ? x : y;
            rh[p] = x < y ? y : x;
            if (!fin(x) || !fin(y))
                return snprintf(msg, cap, "parameter %s: its interval times the nominal value of agent slot %d is not finite", name[p], s), msg;
        }
        for (int p : positive)
            if (d[p].kind != kParamFixed && !(rl[p] > 0.0))
                return snprintf(msg, cap, "parameter %s must stay above 0, its draws reach %g (agent slot %d)", name[p], rl[p], s), msg;
        for (const int(&q)[2] : below)
            if ((d[q[0]].kind != kParamFixed || d[q[1]].kind != kParamFixed) && !(rh[q[0]] < rl[q[1]]))
                return snprintf(msg, cap, "parameter %s must stay below %s, its draws reach %g against %g (agent slot %d)", name[q[0]], name[q[1]],
                                rh[q[0]], rl[q[1]], s), msg;
    }
    return nullptr;
}

}  // namespace f110
