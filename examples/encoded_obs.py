#!/usr/bin/env python3
"""A device-resident loop on compact observations: encode -> policy -> step, nothing crossing PCIe and no host synchronisation
inside it.

    scans [N][1080] float64 (HBM) --f110_obs_encode_device--> stack [N][F][D] float32 (HBM) --MLP--> actions [N][2] (HBM)
                                                                                           --f110_step_device (auto re-seat)--> scans ...

The encoder pools the scan into 108 sectors, appends five state columns and keeps the last four frames; an env that was
re-seated inside a step has its frames refilled by the encode after its first step, which only the simulator can know.  The
policy is a tiny random MLP in PyTorch-ROCm fed through DLPack (`torch.from_dlpack(stack)`, zero copy) on the simulator's own
stream; without torch (or with --no-torch) the built-in scan policy stands in and the encode still runs every step.

    python examples/encoded_obs.py [--envs 4096] [--steps 500] [--no-torch]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch = None
if "--no-torch" not in sys.argv:
    try:
        import torch  # noqa: F401  BEFORE the simulator's library: both then share one libamdhip64.so
        if not torch.cuda.is_available():
            torch = None
    except Exception:  # noqa: BLE001 - no torch here: the built-in policy stands in
        torch = None
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args(argv)
    E, A = args.envs, args.agents
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    start = workload.bench_start_poses(E, A)
    sim.reset(start)
    d_start = sim.device_array((N, 3))
    d_start.upload(start)
    d_resets = sim.device_array((1,), np.int32)
    d_resets.upload(np.zeros(1, np.int32))
    sim.set_auto_reseat(d_start, 0, d_resets)      # crashed envs go back to their start poses inside the step
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    enc = amd.ObsEncoder(sectors=108, pool="min", features=("vx", "steer", "yaw_rate", "slip", "collision"), frames=4,
                         range_clip=10.0, range_scale=10.0, scales={"vx": 8.0, "steer": 0.4189, "yaw_rate": 3.0})
    sim.step_device(actions)                       # the first observation (step_count 1: the first encode fills every frame)
    stack = sim.encode_obs_device(enc)             # float32 [N][4][113], allocated once

    if torch is not None:
        stream = torch.cuda.ExternalStream(sim.device_views()["stream"], device=torch.device("cuda", sim.device_id))
        obs_t = torch.from_dlpack(stack).reshape(N, -1)     # the encoder's own buffer
        act_t = torch.from_dlpack(actions)                   # the buffer f110_step_device reads
        g = torch.Generator(device="cuda").manual_seed(0)
        w1 = torch.randn(obs_t.shape[1], 64, device="cuda", generator=g) * 0.05
        w2 = torch.randn(64, 2, device="cuda", generator=g) * 0.1

        def policy():
            # the encode may have run as two env blocks on two streams; torch sees only the main one.  The fence orders both
            # blocks in front of torch's reads and the next step behind torch's writes.
            sim.fence()
            with torch.cuda.stream(stream):
                out = torch.tanh(torch.tanh(obs_t @ w1) @ w2)
                act_t[:, 0] = (0.4 * out[:, 0]).to(torch.float64)
                act_t[:, 1] = (3.5 + 2.5 * out[:, 1]).to(torch.float64)
    else:
        def policy():
            sim.scan_policy_device(actions)

    t0 = time.perf_counter()
    for _ in range(args.steps):
        policy()                                   # stack (HBM) -> actions (HBM)
        sim.step_device(actions)                   # integrate, scan, collisions, re-seat
        sim.encode_obs_device(enc, stack)          # scans + state (HBM) -> stack (HBM), frames shifted or refilled
    sim.sync()                                     # the only synchronisation: to read the clock
    dt = time.perf_counter() - t0
    frames = stack.download()
    print("%d envs x %d agents, %d steps: %.3f ms per step, %.1f M agent-steps/s; %d env re-seats; stack %s float32, newest frame mean %.4f (%s policy)"
          % (E, A, args.steps, dt / args.steps * 1e3, N * args.steps / dt / 1e6, int(d_resets.download()[0]), frames.shape,
             float(np.nanmean(frames[:, -1, :108])), "torch MLP via DLPack" if torch is not None else "built-in scan"))
    if torch is not None:
        del obs_t, act_t
        torch.cuda.synchronize()
    sim.close()
    return N * args.steps / dt


if __name__ == "__main__":
    main()
