// tests/host_harness/scan_order_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the agent-aligned scan's task order (f1tenth_gym_amd/csrc/f110_math.hpp, scan_task_agent), for
// tests/test_scan_env_order_host.py: the map from task ids to (agent, sector) is checked without a GPU.
#include <cstdint>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// agent[n], sector[n] of the tasks 0 .. n - 1, with the reciprocal the host passes to the kernel
void hh_scan_task_agent(uint32_t n, uint32_t tpa, uint32_t A, uint32_t *agent, uint32_t *sector)
{
    const uint32_t inv = scan_task_inv(A);
    for (uint32_t t = 0; t < n; ++t) scan_task_agent(t, tpa, A, inv, agent[t], sector[t]);
}

// the reciprocal division at its limit: the largest remainders (and those around every multiple of A near the top) of a launch
// with tpa * A * A at the bound scan_task_inv_ok accepts; returns the number of remainders whose quotient is wrong
uint32_t hh_scan_task_inv_errors(uint32_t tpa, uint32_t A)
{
    if (!scan_task_inv_ok(tpa, A)) return 0xffffffffu;
    const uint32_t inv = scan_task_inv(A), top = tpa * A;   // rem < top
    uint32_t bad = 0;
    for (uint32_t k = 0; k < 100000u && k < top; ++k) {
        const uint32_t rems[2] = {k, top - 1u - k};
        for (uint32_t rem : rems) {
            uint32_t agent, sector;
            scan_task_agent(rem, tpa, A, inv, agent, sector);   // env 0: task == rem
            bad += (sector != rem / A || agent != rem % A) ? 1u : 0u;
        }
    }
    return bad;
}

}
