"""test_gpu_rollout.py::test_torch_consumer_in_a_fresh_process, in a process of its own (torch first, then the simulator's library):
the rollout's summary and trajectory through DLPack are float32 tensors over the same memory, equal to the NumPy download, and an
argmax over the candidates picks each car's action where the numbers are."""
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

E, A, K, H = 16, 2, 6, 4
N = E * A
s = amd.BatchSim(num_envs=E, num_agents=A)
s.set_map_image(*load_map_image("example_map"))
s.set_track(amd.Track.from_csv(os.path.join(MAPS, "example_waypoints.csv")))
s.reset(bench_start_poses(E, A))
lib = np.array([[[st, 3.0]] * H for st in np.linspace(-0.4, 0.4, K)])
p = amd.Rollout(k=K, horizon=H, repeat=5, channels=("alive", "min_clear", "progress"), margin=0.3, traj=True)   # (the output's order)
d_lib = s.device_array(lib.shape); d_lib.upload(lib)
act = s.device_array((N, 2)); act.upload(np.tile([0.0, 2.0], (N, 1)))
buf, tr = s.device_array(p.shape(N), np.float32), s.device_array(p.traj_shape(N), np.float32)
for _ in range(6):
    s.step_device(act)
    s.rollout_device(p, d_lib, buf, tr)
    s.sync()
    t, tt = torch.from_dlpack(buf), torch.from_dlpack(tr)
    score = t[:, :, 2] - 0.5 * (20.0 - t[:, :, 0])
    best = score.argmax(dim=1)
    a = torch.from_dlpack(d_lib)[best, 0, :].contiguous()
    act.upload(a.cpu().numpy())
assert t.dtype == torch.float32 and tuple(t.shape) == (N, K, 3) and t.is_contiguous() and t.device.type == "cuda" and t.data_ptr() == buf.ptr
assert tuple(tt.shape) == (N, K, H, 4) and tt.data_ptr() == tr.ptr
host, htr = buf.download(), tr.download()
assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)) and np.array_equal(tt.cpu().numpy().view(np.uint32), htr.view(np.uint32))
# on the raceline at 3 m/s nothing dies within 20 steps; every candidate gains ground and ends ahead of the car in its own frame
assert np.all(host[..., 0] == 20.0) and np.all(host[..., 1] > 0.3) and np.all(host[..., 2] > 0.0) and np.all(htr[:, :, -1, 0] > 0.0)
assert tuple(a.shape) == (N, 2) and bool((a[:, 1] == 3.0).all())
del t, tt, score, best, a
torch.cuda.synchronize()
s.close()
print("ROLLOUT TORCH OK")
