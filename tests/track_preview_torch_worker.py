"""test_gpu_track_preview.py::test_torch_consumer_in_a_fresh_process, in a process of its own (torch first, then the simulator's
library): the preview through DLPack is a float32 [N, P, D] tensor over the same memory, equal to the NumPy download, and a
pure-pursuit-like steering rule reads it where it is."""
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
s.set_track(amd.Track.from_csv(os.path.join(MAPS, "example_waypoints.csv"), attrs={"vx": 5}))
s.enable_track()
s.reset(bench_start_poses(E, A))
p = amd.TrackPreview(points=8, channels=("x", "y", "attr0"), frame="ego")
act = s.device_array((N, 2)); act.upload(np.tile([0.0, 2.0], (N, 1)))
buf = s.device_array(p.shape(N), np.float32)
for _ in range(6):
    s.step_device(act)
    s.track_preview_device(p, buf)
    s.sync()
    t = torch.from_dlpack(buf)
    look = t[:, 3]                                              # the station 2 m ahead: x, y in the car's frame, the raceline's speed
    steer = torch.atan(2.0 * 0.33 * look[:, 1] / (look[:, 0] ** 2 + look[:, 1] ** 2)).clamp(-0.4189, 0.4189)
    a = torch.stack([steer.double(), look[:, 2].double() * 0.5], dim=1).contiguous()
    act.upload(a.cpu().numpy())
assert t.dtype == torch.float32 and tuple(t.shape) == (N, 8, 3) and t.is_contiguous() and t.device.type == "cuda"
assert t.data_ptr() == buf.ptr
host = buf.download()
assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32))
# cars that started on the line and followed it for six steps: station 0 is 0.5 m of arc away, ahead of the car
assert np.all(host[:, 0, 0] > 0.0) and np.all(np.hypot(host[:, 0, 0], host[:, 0, 1]) < 0.6)
assert np.all(host[:, :, 2] > 0.0)                                             # the raceline's speed profile is positive
del t, look, steer, a
torch.cuda.synchronize()
s.close()
print("TRACK PREVIEW TORCH OK")
