// tests/host_harness/param_sampler_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the parameter sampler's draw and of its interval check (f1tenth_gym_amd/csrc/f110_rng.hpp, param_*),
// for tests/test_param_sampler_host.py: the check and the draw are compared with the Python model (tests/param_sampler_ref.py)
// and with ParamSampler.validate without a GPU.  The GPU tests hold the device instantiation (and the kernel around it) to the
// same model.  With -DPARAM_HARNESS_MAIN the file is a stand-alone program that runs the refusals and one draw against values
// the NumPy model printed (what the address and undefined-behaviour sanitizers are run on).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_rng.hpp"

using namespace f110;

extern "C" {

// entries [18] in f110_param_dist's layout; nominal [A][18].  0: may be armed; 1: refused, the reason in msg
int hh_param_check(const ParamDist *entries, const double *nominal, int A, char *msg, int cap)
{
    return param_dists_check(entries, nominal, A, msg, (size_t)cap) ? 1 : 0;
}

// m envs of A agents drawn `rounds` times: streams [m][4] in and out, out [rounds][m * A][18] (a round starts from the rows before
// it, round 0 from the nominal ones).  The caller has checked the entries.
void hh_param_draw(const ParamDist *entries, const double *nominal, int A, uint64_t *streams, int m, int rounds, double *out)
{
    const ZigTables zt = {kZigK, kZigW, kZigF};
    const size_t per_env = (size_t)A * NPARAMS, per_round = per_env * m;
    for (int r = 0; r < rounds; ++r)
        for (int e = 0; e < m; ++e) {
            double *rows = out + per_round * r + per_env * e;
            std::memcpy(rows, r ? rows - per_round : nominal, sizeof(double) * per_env);
            uint64_t *w = streams + 4 * (size_t)e;
            U128 st = {w[0], w[1]};
            param_draw_env(entries, nominal, A, st, U128{w[2], w[3]}, zt, rows);
            w[0] = st.hi;
            w[1] = st.lo;
        }
}

}

#ifdef PARAM_HARNESS_MAIN
static ParamDist fixed() { return ParamDist{kParamFixed, kParamScopeAgent, 0.0, 0.0, 0.0, 0.0, 0, 0}; }
static ParamDist uni(double a, double b, int scope, int rel) { return ParamDist{kParamUniform, scope, a, b, 0.0, 0.0, rel, 0}; }
static ParamDist nor(double a, double b, double lo, double hi, int scope, int rel) { return ParamDist{kParamNormal, scope, a, b, lo, hi, rel, 0}; }

// every refusal of include/f110.h, each naming its parameter; then two envs of two agents drawn twice with
// mu ~ U(0.5, 1.1) per env, m ~ 1 +- 15 % of the nominal per agent, C_Sf ~ N(4.7, 0.5) clipped to [4.5, 5.0] per agent, against
// tests/param_sampler_ref.py's rows for PCG64(SeedSequence(2024, spawn_key=(e,))), e = 3, 4
int main()
{
    const double P[NPARAMS] = {1.0489, 4.718, 5.4562, 0.15875, 0.17145, 0.074, 3.74, 0.04712, -0.4189, 0.4189, -3.2, 3.2, 7.319, 9.51, -5.0, 20.0, 0.31, 0.58};
    const int A = 2;
    double nominal[A * NPARAMS];
    for (int s = 0; s < A; ++s)
        for (int p = 0; p < NPARAMS; ++p) nominal[s * NPARAMS + p] = P[p] * (p == P_M && s == 1 ? 1.25 : 1.0);
    struct Bad { int p; ParamDist d; const char *name; };
    const Bad bad[] = {
        {P_WIDTH, uni(0.3, 0.4, 0, 0), "width"},
        {P_LENGTH, nor(0.58, 0.0, 0.5, 0.6, 0, 0), "length"},
        {P_MU, uni(1.1, 0.5, 0, 0), "mu"},
        {P_MU, uni(NAN, 0.5, 0, 0), "mu"},
        {P_CSF, uni(4.0, INFINITY, 0, 0), "C_Sf"},
        {P_M, nor(3.7, -0.1, 3.0, 4.0, 0, 0), "m"},
        {P_M, nor(3.7, 0.1, -INFINITY, 4.0, 0, 0), "m"},
        {P_M, nor(3.7, 0.1, 4.0, 3.0, 0, 0), "m"},
        {P_MU, uni(0.0, 1.0, 1, 0), "mu"},
        {P_I, uni(-0.5, 1.5, 0, 1), "I"},
        {P_AMAX, nor(9.0, 1.0, -1.0, 12.0, 0, 0), "a_max"},
        {P_VSWITCH, uni(0.0, 8.0, 0, 0), "v_switch"},
        {P_SMIN, uni(-0.5, 0.5, 0, 0), "s_min"},
        {P_SMAX, uni(-0.5, 0.5, 0, 0), "s_max"},
        {P_SVMAX, uni(0.5, 1.5, 0, 1), "sv_max"},   // fine on its own: see below
        {P_SVMIN, uni(-1.5, 1.0, 0, 1), "sv_min"},
        {P_VMAX, uni(-6.0, 20.0, 0, 0), "v_max"},
        {P_MU, ParamDist{7, 0, 0.5, 1.0, 0.0, 0.0, 0, 0}, "mu"},
        {P_MU, ParamDist{kParamUniform, 5, 0.5, 1.0, 0.0, 0.0, 0, 0}, "mu"},
    };
    char msg[256];
    int n_bad = 0;
    for (const Bad &b : bad) {
        ParamDist d[NPARAMS];
        for (int p = 0; p < NPARAMS; ++p) d[p] = fixed();
        d[b.p] = b.d;
        const int rc = hh_param_check(d, nominal, A, msg, (int)sizeof msg);
        const bool fine = b.p == P_SVMAX;   // sv_max in 0.5 .. 1.5 of 3.2 stays above sv_min = -3.2
        if (rc != (fine ? 0 : 1)) return printf("refusal %d (%s): rc = %d\n", n_bad, b.name, rc), 1;
        if (!fine && !std::strstr(msg, b.name)) return printf("refusal %d: '%s' does not name %s\n", n_bad, msg, b.name), 2;
        ++n_bad;
    }
    ParamDist d[NPARAMS];
    for (int p = 0; p < NPARAMS; ++p) d[p] = fixed();
    d[P_MU] = uni(0.5, 1.1, kParamScopeEnv, 0);
    d[P_CSF] = nor(4.7, 0.5, 4.5, 5.0, kParamScopeAgent, 0);
    d[P_M] = uni(0.85, 1.15, kParamScopeAgent, 1);
    if (hh_param_check(d, nominal, A, msg, (int)sizeof msg)) return printf("the draw's entries were refused: %s\n", msg), 3;
    const int m = 2, rounds = 2;
    // printed by the model: the words before, (mu, C_Sf, m) of every row after each round, the words after
    const uint64_t kWords[4 * m] = {0x895cc647e7ce3e5eULL, 0xbc656ea4b2120959ULL, 0x7a24bc7cad695a9cULL, 0xb1308cf8608cf887ULL,
                                    0x67e77c57ae6acae2ULL, 0xe4fca61db360d3a1ULL, 0xca5382809e488d2eULL, 0x55829e4ca2b3f165ULL};
    const double kExpect[rounds][m * A][3] = {
        {{0x1.187372496f56cp-1, 0x1.234913c9092dcp+2, 0x1.12e256c886832p+2}, {0x1.187372496f56cp-1, 0x1.2000000000000p+2, 0x1.382ebd52feb0ep+2},
         {0x1.fe0ba921ce670p-1, 0x1.3e5a170f224c4p+2, 0x1.d8e1d830e0ce3p+1}, {0x1.fe0ba921ce670p-1, 0x1.3411aac2c8fe0p+2, 0x1.2636e39e2effcp+2}},
        {{0x1.e551a2efaa214p-1, 0x1.2000000000000p+2, 0x1.a05e95cfe412ep+1}, {0x1.e551a2efaa214p-1, 0x1.21bbf969397afp+2, 0x1.141797fad3312p+2},
         {0x1.6c127fe2f5ce1p-1, 0x1.2000000000000p+2, 0x1.b1532806b5fc1p+1}, {0x1.6c127fe2f5ce1p-1, 0x1.2000000000000p+2, 0x1.12ce33233d6ffp+2}},
    };
    const uint64_t kWordsAfter[4 * m] = {0x59510bf062591d1aULL, 0x1680792ed2969b03ULL, 0x7a24bc7cad695a9cULL, 0xb1308cf8608cf887ULL,
                                         0x6b00014e2ed5ca85ULL, 0x31cf2290c63c794fULL, 0xca5382809e488d2eULL, 0x55829e4ca2b3f165ULL};
    uint64_t streams[4 * m];
    std::memcpy(streams, kWords, sizeof streams);
    std::vector<double> out((size_t)rounds * m * A * NPARAMS);
    hh_param_draw(d, nominal, A, streams, m, rounds, out.data());
    for (int r = 0; r < rounds; ++r)
        for (int i = 0; i < m * A; ++i) {
            const double *row = &out[((size_t)r * m * A + i) * NPARAMS];
            const double got[3] = {row[P_MU], row[P_CSF], row[P_M]};
            if (std::memcmp(got, kExpect[r][i], sizeof got) != 0)
                return printf("round %d agent %d: %a %a %a, the model has %a %a %a\n", r, i, got[0], got[1], got[2], kExpect[r][i][0], kExpect[r][i][1], kExpect[r][i][2]), 4;
            for (int p = 0; p < NPARAMS; ++p)
                if (p != P_MU && p != P_CSF && p != P_M && row[p] != nominal[(i % A) * NPARAMS + p]) return printf("a fixed slot moved\n"), 5;
        }
    if (std::memcmp(streams, kWordsAfter, sizeof streams) != 0) return printf("the streams ended elsewhere\n"), 6;
    printf("param sampler harness: ok (%d refusals, %d rows)\n", n_bad - 1, rounds * m * A);
    return 0;
}
#endif
