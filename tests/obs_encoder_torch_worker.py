"""test_gpu_obs_encoder.py::test_torch_consumer_in_a_fresh_process, in a process of its own (torch first, then the simulator's
library): the encoder's stack through DLPack is a float32 [N, F, D] tensor over the same memory, equal to the NumPy download."""
import os
import sys

try:
    import torch
except Exception as ex:  # noqa: BLE001
    print("SKIP torch is not importable: %s" % ex)
    sys.exit(0)
if not torch.cuda.is_available():
    print("SKIP this torch build sees no GPU")
    sys.exit(0)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import f1tenth_gym_amd as amd  # noqa: E402
from _util import bench_start_poses, load_map_image  # noqa: E402

E, A = 16, 2
N = E * A
s = amd.BatchSim(num_envs=E, num_agents=A)
s.set_map_image(*load_map_image("example_map"))
s.set_noise_rng(12345, 0.01)
s.reset(bench_start_poses(E, A))
enc = amd.ObsEncoder(sectors=108, pool="min", features=("vx", "steer", "yaw_rate", "slip", "collision"), frames=4)
act = s.device_array((N, 2)); act.upload(np.tile([0.1, 3.0], (N, 1)))
stack = None
for _ in range(6):
    s.step_device(act)
    stack = s.encode_obs_device(enc, stack)
t = torch.from_dlpack(stack)
assert t.dtype == torch.float32 and tuple(t.shape) == (N, 4, 113) and t.is_contiguous() and t.device.type == "cuda"
assert t.data_ptr() == stack.ptr
host = stack.download()
assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32))
assert not np.array_equal(host[:, 0], host[:, 3])          # the frames differ: the cars are moving
# a policy network reads it where it is
net = torch.nn.Sequential(torch.nn.Linear(4 * 113, 32), torch.nn.Tanh(), torch.nn.Linear(32, 2)).to(t.device)
with torch.no_grad():
    y = net(t.reshape(N, -1))
assert tuple(y.shape) == (N, 2) and bool(torch.isfinite(y).all())
del t, y
torch.cuda.synchronize()
s.close()
print("OBS ENCODER TORCH OK")
