"""test_gpu_neighbors.py::test_torch_consumer_in_a_fresh_process, in a process of its own (torch first, then the simulator's
library): the neighbours through DLPack are a float32 [N, K, D] tensor over the same memory, equal to the NumPy download, and a
rule that brakes behind the nearest car ahead reads them where they are."""
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
from _util import MAPS, bench_start_poses, load_map_image  # noqa: E402

E, A = 16, 2
N = E * A
s = amd.BatchSim(num_envs=E, num_agents=A)
s.set_map_image(*load_map_image("example_map"))
s.set_noise_rng(12345, 0.01)
s.set_track(amd.Track.from_csv(os.path.join(MAPS, "example_waypoints.csv")))
s.enable_track()
s.reset(bench_start_poses(E, A))
p = amd.Neighbors(k=1, channels=("dx", "dy", "dist", "gap_s", "valid"), max_range=10.0)
act = s.device_array((N, 2)); act.upload(np.tile([0.0, 2.0], (N, 1)))
buf = s.device_array(p.shape(N), np.float32)
for _ in range(6):
    s.step_device(act)
    s.neighbors_device(p, buf)
    s.sync()
    t = torch.from_dlpack(buf)
    near = t[:, 0]                                              # the nearest opponent: dx, dy, dist, gap_s, valid
    ahead = (near[:, 4] > 0) & (near[:, 0] > 0) & (near[:, 1].abs() < 1.0)
    speed = torch.where(ahead, (near[:, 2] - 0.5).clamp(0.0, 3.0), torch.full_like(near[:, 2], 3.0))
    a = torch.stack([torch.zeros_like(speed).double(), speed.double()], dim=1).contiguous()
    act.upload(a.cpu().numpy())
assert t.dtype == torch.float32 and tuple(t.shape) == (N, 1, 5) and t.is_contiguous() and t.device.type == "cuda"
assert t.data_ptr() == buf.ptr
host = buf.download()
assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32))
# two cars per env, started ten waypoints (about 1 m) apart on the line: each sees the other, the same distance away, the leader behind
# it and the follower ahead, and the gaps along the track are opposite
h = host.reshape(E, A, 5)
assert np.all(h[..., 4] == 1.0) and np.array_equal(h[:, 0, 2], h[:, 1, 2]) and np.all(h[..., 2] < 3.0)
assert np.all(h[:, 0, 0] < 0.0) and np.all(h[:, 1, 0] > 0.0)
assert np.all(h[:, 0, 3] < 0.0) and np.all(h[:, 1, 3] > 0.0) and np.allclose(h[:, 0, 3], -h[:, 1, 3], atol=1e-5)
assert bool(ahead.reshape(E, A)[:, 1].all()) and not bool(ahead.reshape(E, A)[:, 0].any())
del t, near, ahead, speed, a
torch.cuda.synchronize()
s.close()
print("NEIGHBORS TORCH OK")
