"""BatchSim — the thin Python owner of one libf110_hip handle (one MI355X, one HIP stream).

E independent environments x A agents are stepped in lockstep on the device.  This class only
marshals NumPy arrays to the C ABI (include/f110.h); all arithmetic happens in the HIP kernels.
The reference-compatible façades (Simulator, ScanSimulator2D, F110Env) are built on it.
"""
import ctypes as C
import os
import types
import weakref

import numpy as np

from . import _ffi
from ._ffi import check, as_f64, dptr, i32ptr, u64ptr
from ._spec import is_int

DEFAULT_PARAMS = {'mu': 1.0489, 'C_Sf': 4.718, 'C_Sr': 5.4562, 'lf': 0.15875, 'lr': 0.17145,
                  'h': 0.074, 'm': 3.74, 'I': 0.04712, 's_min': -0.4189, 's_max': 0.4189,
                  'sv_min': -3.2, 'sv_max': 3.2, 'v_switch': 7.319, 'a_max': 9.51,
                  'v_min': -5.0, 'v_max': 20.0, 'width': 0.31, 'length': 0.58}  # f110_env.py:130


def trig_tables(theta_dis):
    """laser_models.py:379-381 — NumPy-computed so the device table is bit-identical."""
    theta_arr = np.linspace(0.0, 2 * np.pi, num=theta_dis)
    return np.sin(theta_arr), np.cos(theta_arr)


def beam_tables(num_beams, fov, params):
    """RaceCar's class-level per-beam tables, base_classes.py:125-158: beam angles (built by a
    Python loop, not linspace), their cosines, and the lidar-to-body-edge distance."""
    incr = fov / (num_beams - 1)
    scan_angles = np.zeros((num_beams,))
    cosines = np.zeros((num_beams,))
    side_distances = np.zeros((num_beams,))
    dist_sides = params['width'] / 2.
    dist_fr = (params['lf'] + params['lr']) / 2.
    half_pi = np.pi / 2
    for i in range(num_beams):
        angle = -fov / 2. + i * incr
        scan_angles[i] = angle
        cosines[i] = np.cos(angle)
        with np.errstate(divide='ignore'):      # a beam at angle 0 exactly divides by -0.0: side distance -inf, as in the reference, without its warning
            to_side, to_fr = _edge_distances(angle, dist_sides, dist_fr, half_pi)
        side_distances[i] = min(to_side, to_fr)
    return scan_angles, cosines, side_distances


def _edge_distances(angle, dist_sides, dist_fr, half_pi):
    """from the lidar along a beam to the car's side and to its front / rear edge (base_classes.py:139-156)"""
    if angle > 0:
        if angle < half_pi:
            return dist_sides / np.sin(angle), dist_fr / np.cos(angle)
        return dist_sides / np.cos(angle - np.pi / 2.), dist_fr / np.sin(angle - np.pi / 2.)
    if angle > -half_pi:
        return dist_sides / np.sin(-angle), dist_fr / np.cos(-angle)
    return dist_sides / np.cos(-angle - np.pi / 2), dist_fr / np.sin(-angle - np.pi / 2)


def load_map_files(map_path, map_ext):
    """ScanSimulator2D.set_map's file handling, laser_models.py:397-416: <stem><ext> image +
    yaml with 'resolution' and 'origin'.  Returns (uint8 image top-row-first, resolution, origin)."""
    from . import mapio   # stdlib zlib + NumPy: the box needs neither PIL nor PyYAML
    map_img_path = os.path.splitext(map_path)[0] + map_ext

    def pil_image():
        from PIL import Image
        with Image.open(map_img_path) as im:
            arr = np.array(im)
        if arr.dtype == np.bool_:
            # 1-bit images: PIL hands out booleans and the reference's astype(float64) sees 0. / 1. — every cell is <= 128 and
            # becomes an obstacle (laser_models.py:399-404).  Reproduced as it is (bit parity), with a warning: the map is
            # degenerate in the reference too; convert the image to 8-bit grayscale.
            import warnings
            warnings.warn("%s is a 1-bit image: like the reference, every cell thresholds to 'occupied' (values 0 / 1 <= 128); "
                          "save the map as 8-bit grayscale" % map_img_path)
            arr = arr.astype(np.uint8)
        if arr.ndim != 2:
            raise ValueError("map image must be single-channel grayscale, got shape %s" % (arr.shape,))
        return arr
    if map_img_path.lower().endswith(".png"):
        try:
            img = mapio.read_png_gray(map_img_path)
        except ValueError as ex:   # palette / 1-2-4-bit / interlaced PNGs: what the reference hands to PIL, if PIL is here
            try:
                img = pil_image()
            except ImportError:
                raise ex
    else:   # any other image format the reference would hand to PIL: PIL it is, if installed
        img = pil_image()
    if img.dtype != np.uint8:
        # the reference thresholds the decoded values at 128 (laser_models.py:403-404)
        img = np.where(img.astype(np.float64) > 128., 255, 0).astype(np.uint8)
    try:
        meta = mapio.read_map_yaml(map_path)
    except ValueError as ex:   # block-style lists / nested keys: yaml.safe_load like the reference (:410-416), if PyYAML is here
        try:
            import yaml
        except ImportError:
            raise ex
        with open(map_path) as f:
            meta = yaml.safe_load(f)
    return np.ascontiguousarray(img), float(meta['resolution']), [float(v) for v in meta['origin']]


from . import _dlpack  # noqa: E402


class DeviceArray(object):
    """A device buffer owned by a BatchSim handle (exposes __cuda_array_interface__ so torch /
    cupy can wrap it without a copy; ROCm uses the same protocol)."""

    def __init__(self, sim, shape, dtype=np.float64, ptr=None):
        self.sim = sim
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._owned = ptr is None
        if ptr is None:
            p = C.c_void_p()
            check(_ffi.lib().f110_device_alloc(sim._h, self.nbytes, C.byref(p)), sim._h)
            ptr = p.value
        self.ptr = ptr
        # an owned buffer is returned to the device when the array is collected, on `with` exit, or by
        # free() — whichever comes first; never after its handle is gone (the handle frees nothing of ours,
        # but f110_device_free needs it alive: BatchSim.close() runs the outstanding finalisers first)
        self._fin = None
        if self._owned:
            holder = []
            self._fin = weakref.finalize(self, DeviceArray._release, sim, ptr, holder)
            holder.append(self._fin)
            sim._device_arrays.add(self._fin)

    @staticmethod
    def _release(sim, ptr, holder=None):
        if holder:                       # the finaliser takes itself off the handle's list (no growth in long loops)
            sim._device_arrays.discard(holder[0])
        if sim._h and ptr:
            _ffi.lib().f110_device_free(sim._h, ptr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2}

    # ---- DLPack (the neutral zero-copy hand-off: torch.from_dlpack(arr), cupy.from_dlpack(arr), jax ... — no type of this
    # package crosses the boundary).  kDLROCM = 10; C-contiguous (strides = NULL); the capsule keeps this array alive until
    # the consumer's deleter runs.
    def __dlpack_device__(self):
        return (_dlpack.kDLROCM, int(getattr(self.sim, "device_id", 0)))

    def __dlpack__(self, stream=None, max_version=None, dl_device=None, copy=None):
        """stream = -1: no synchronisation (the caller orders its work against device_views()['stream'] itself); anything
        else: the handle's stream is drained first, so the consumer sees finished data whatever stream it uses.
        max_version / dl_device / copy: the newer protocol's keywords — a version-0 ("dltensor") capsule is what this producer
        makes whatever max_version says (consumers accept it), the data cannot leave its device and is never copied.
        Lifetime: the tensor a consumer makes of the capsule views the simulator's memory; BatchSim.close() refuses to free it
        while such a tensor is alive (drop the tensors first, or close(force=True))."""
        if self.ptr is None:
            raise ValueError("the buffer has been freed")
        if copy is True:
            raise BufferError("DeviceArray.__dlpack__ cannot copy (copy=True): it exports the simulator's own buffer")
        if dl_device is not None and tuple(int(v) for v in dl_device) != self.__dlpack_device__():
            raise BufferError("DeviceArray lives on %s and cannot be exported to dl_device=%s" % (self.__dlpack_device__(), tuple(dl_device)))
        if stream != -1 and getattr(self.sim, "_h", None):
            self.sim.sync()
        return _dlpack.make_capsule(self)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.nbytes != self.nbytes:
            raise ValueError("size mismatch")
        check(_ffi.lib().f110_memcpy_h2d(self.sim._h, self.ptr, host.ctypes.data, self.nbytes), self.sim._h)

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(_ffi.lib().f110_memcpy_d2h(self.sim._h, out.ctypes.data, self.ptr, self.nbytes), self.sim._h)
        return out

    def download_part(self, first_row, n_rows):
        """rows [first_row, first_row + n_rows) along the leading axis (a receive buffer of many ranks' blocks is
        read back one block at a time instead of as one multi-GB host array)"""
        first_row, n_rows = int(first_row), int(n_rows)
        if first_row < 0 or n_rows < 0 or first_row + n_rows > self.shape[0]:
            raise IndexError("rows [%d, %d) are outside an array of %d rows" % (first_row, first_row + n_rows, self.shape[0]))
        row_bytes = (int(np.prod(self.shape[1:])) if len(self.shape) > 1 else 1) * self.dtype.itemsize
        out = np.empty((int(n_rows),) + self.shape[1:], dtype=self.dtype)
        check(_ffi.lib().f110_memcpy_d2h(self.sim._h, out.ctypes.data, self.ptr + int(first_row) * row_bytes, out.nbytes), self.sim._h)
        return out

    def free(self):
        if self._fin is not None:
            self.sim._device_arrays.discard(self._fin)
            self._fin()          # runs at most once
        self.ptr = None


# the 256-byte header of a state blob (include/f110.h, f110_state_*)
STATE_HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("k", "<i4"), ("A", "<i4"), ("B", "<i4"), ("flags", "<i4"),
                         ("cols", "<u4"), ("noise_mode", "<i4"), ("noise_rows", "<i4"), ("n_maps", "<i4"), ("ego_idx", "<i4"),
                         ("max_step", "<i8"), ("noise_id", "<u8", (4,)), ("std_dev", "<f8"), ("total_bytes", "<u8"),
                         ("reserved", "<u8", (19,))])
assert STATE_HEADER.itemsize == _ffi.STATE_HEADER_BYTES
STATE_MAGIC = b"F110SNAP"
STATE_COLUMNS = {"agent": 1, "scans": 2, "rng": 4, "rng_seed": 8, "episode": 16, "params": 32, "env_map": 64, "reset_rng": 128}
# ... and the parameter sampler's stream column, which a handle has next to "params" and never together with set_params_batch's
# rows: not every column of both tables can be active on one handle
STATE_COLUMNS_SAMPLED = {"param_rng": 256}
NOISE_MODES = ("off", "table", "shared_rng", "per_agent_rng")


class StateBlob(object):
    """An exact snapshot of simulator state (BatchSim.save_state / save_envs): `data` is the blob as a NumPy uint8 buffer,
    `header` its parsed header (a dict).  It holds state, not configuration: the maps, tables, per-slot params and noise
    source must already be set on the handle it is loaded into (the load refuses a blob that does not fit)."""

    def __init__(self, data):
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data)
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("a state blob is a 1-D uint8 buffer")
        if data.nbytes < STATE_HEADER.itemsize:
            raise ValueError("a state blob is at least %d bytes (got %d)" % (STATE_HEADER.itemsize, data.nbytes))
        h = data[:STATE_HEADER.itemsize].view(STATE_HEADER)[0]
        if bytes(h["magic"]) != STATE_MAGIC:
            raise ValueError("not a simulator state blob (bad magic %r)" % bytes(h["magic"]))
        if int(h["version"]) != _ffi.STATE_VERSION:
            raise ValueError("state blob format version %d, this package reads version %d" % (int(h["version"]), _ffi.STATE_VERSION))
        if int(h["total_bytes"]) != data.nbytes:
            raise ValueError("state blob of %d bytes, its header says %d" % (data.nbytes, int(h["total_bytes"])))
        cols = int(h["cols"])
        self.data = data
        self.header = {
            "version": int(h["version"]), "num_envs": int(h["k"]), "num_agents": int(h["A"]), "num_beams": int(h["B"]),
            "scans": bool(int(h["flags"]) & _ffi.STATE_SCANS), "columns": tuple(n for n, b in list(STATE_COLUMNS.items()) + list(STATE_COLUMNS_SAMPLED.items()) if cols & b),
            "noise_mode": NOISE_MODES[int(h["noise_mode"])] if 0 <= int(h["noise_mode"]) < len(NOISE_MODES) else int(h["noise_mode"]),
            "noise_rows": int(h["noise_rows"]), "noise_id": tuple(int(v) for v in h["noise_id"]), "std_dev": float(h["std_dev"]),
            "n_maps": int(h["n_maps"]), "ego_idx": int(h["ego_idx"]), "max_step": int(h["max_step"]), "total_bytes": int(h["total_bytes"])}

    @property
    def num_envs(self):
        return self.header["num_envs"]

    @property
    def nbytes(self):
        return self.data.nbytes

    def to_bytes(self):
        return self.data.tobytes()

    @classmethod
    def from_bytes(cls, raw):
        return cls(np.frombuffer(bytes(raw), dtype=np.uint8).copy())

    def __repr__(self):
        h = self.header
        return "StateBlob(%d envs x %d agents, %d beams, columns=%s, %d bytes)" % (
            h["num_envs"], h["num_agents"], h["num_beams"], ",".join(h["columns"]), h["total_bytes"])


def _with_extras(out, *optional):
    """a unit form's result: `out` alone, or a tuple of it and the optional outputs that were asked for (not None)"""
    res = (out,) + tuple(x for x in optional if x is not None)
    return res[0] if len(res) == 1 else res


class BatchSim(object):
    def __init__(self, params=None, num_envs=1, num_agents=2, num_beams=1080, fov=4.7, eps=0.0001,
                 theta_dis=2000, max_range=30.0, time_step=0.01, integrator=_ffi.INTEGRATOR_RK4,
                 lidar_dist=0.0, ttc_thresh=0.005, device_id=0, map_layout=_ffi.MAP_DEFAULT,
                 scan_block=0, scan_tasks_per_wave=0, step_groups=0, step_graph=0, exp=None):
        self._h = None
        self._device_arrays = set()   # finalisers of the DeviceArrays this handle owns memory for
        self._obs_stacks = {}         # encode_obs_device(out=None): id(encoder) -> (encoder, its stack)
        L = _ffi.lib()
        self.params = dict(DEFAULT_PARAMS if params is None else params)
        self.E, self.A, self.B = int(num_envs), int(num_agents), int(num_beams)
        self.N = self.E * self.A
        self.fov, self.theta_dis, self.time_step = float(fov), int(theta_dis), float(time_step)
        self.device_id = int(device_id)
        cfg = _ffi.Config()
        cfg.abi_version = _ffi.ABI_VERSION
        cfg.num_envs, cfg.num_agents, cfg.num_beams = self.E, self.A, self.B
        cfg.theta_dis, cfg.integrator, cfg.device_id = self.theta_dis, int(integrator), self.device_id
        cfg.map_layout, cfg.scan_block = int(map_layout), int(scan_block)
        cfg.scan_tasks_per_wave = int(scan_tasks_per_wave)
        cfg.step_groups = int(step_groups)
        cfg.step_graph = int(step_graph)
        cfg.fov, cfg.eps, cfg.max_range = float(fov), float(eps), float(max_range)
        cfg.time_step, cfg.lidar_dist, cfg.ttc_thresh = float(time_step), float(lidar_dist), float(ttc_thresh)
        pv = _ffi.params_vector(self.params)
        for i in range(_ffi.NPARAMS):
            cfg.params[i] = pv[i]
        self._slot_rows = np.tile(np.asarray(pv, dtype=np.float64), (self.A, 1))   # the agent slots' parameter sets (set_params)
        h = C.c_void_p()
        check(L.f110_create(C.byref(cfg), C.byref(h)), None)
        self._h = h.value
        self._f_step_host = _ffi.lib().f110_step_host
        # NumPy-computed tables (bit-identical to the reference's)
        s, c = trig_tables(self.theta_dis)
        check(L.f110_set_trig_tables(self._h, dptr(s), dptr(c), self.theta_dis), self._h)
        self.scan_angles, self.cosines, self.side_distances = beam_tables(self.B, self.fov, self.params)
        check(L.f110_set_beam_tables(self._h, dptr(self.scan_angles), dptr(self.cosines),
                                     dptr(self.side_distances), self.B), self._h)
        self.has_map = False
        self.noise_rows = 0
        # experimental build only (libf110_hip_exp.so, F110_LIB_VARIANT=experimental): A/B switches, from the
        # `exp` argument and from F110_EXP="key=value,key=value" — read here, by the host; the library itself
        # reads no environment variable.  The product library refuses every key (ExperimentalOnly).
        switches = dict(kv.split("=", 1) for kv in os.environ.get("F110_EXP", "").split(",") if "=" in kv)
        switches.update(exp or {})
        for key, val in switches.items():
            self.exp_set(key, int(val))

    def exp_set(self, key, value):
        check(_ffi.lib().f110_exp_set(self._h, str(key).encode(), int(value)), self._h)

    # ------------------------------------------------------------------ lifetime
    def close(self, force=False):
        """frees the handle and every device buffer it owns.  Refused (BufferError) while a DLPack consumer still holds one of
        them (a torch tensor made by from_dlpack would point at freed memory): drop those tensors first, or force=True"""
        if self._h:
            if not force and _dlpack.exports_of(self):
                raise BufferError("%d DLPack export(s) of this simulator's buffers are still alive; delete the tensors made from "
                                  "them before close(), or close(force=True)" % _dlpack.exports_of(self))
            for fin in list(self._device_arrays):   # device buffers still alive: give them back first
                fin()
            self._device_arrays.clear()
            # pinned host blocks (pinned_empty) belong to the NumPy arrays that view them: each block is
            # unpinned and freed when its last view is collected, which may be after this handle is gone
            _ffi.lib().f110_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                self.close(force=True)
            except _ffi.F110LibraryError as ex:   # interpreter teardown: report, do not raise from a finaliser
                import sys
                print("BatchSim.__del__: %s" % ex, file=sys.stderr)

    def sync(self):
        check(_ffi.lib().f110_sync(self._h), self._h)

    def fence(self):
        """f110_stream_fence: call between this handle's calls and EXTERNAL work on device_views()['stream'] (torch / cupy on an
        ExternalStream around it): the handle's work in flight — both env blocks of a two-block step — is ordered in front of
        that work, and the next step runs behind it.  Never blocks the host."""
        check(_ffi.lib().f110_stream_fence(self._h), self._h)

    # ------------------------------------------------------------------ configuration
    def set_map(self, map_path, map_ext):
        img, res, origin = load_map_files(map_path, map_ext)
        self.set_map_image(img, res, origin)

    def add_map(self, map_path, map_ext):
        """register another track from its yaml + image files; returns its slot (set_env_maps)"""
        img, res, origin = load_map_files(map_path, map_ext)
        return self.add_map_image(img, res, origin)

    def set_map_image(self, img_top_first, resolution, origin):
        img = np.ascontiguousarray(img_top_first, dtype=np.uint8)
        if img.ndim != 2:
            raise ValueError("map image must be 2-D")
        check(_ffi.lib().f110_set_map_image(self._h, img.ctypes.data_as(_ffi._u8p), img.shape[0], img.shape[1],
                                            float(resolution), float(origin[0]), float(origin[1]),
                                            float(origin[2])), self._h)
        self.has_map = True
        self.map_resolution, self.map_origin = float(resolution), list(origin)

    def set_map_dt(self, dt, resolution, origin):
        dt = as_f64(dt)
        if dt.ndim != 2:
            raise ValueError("distance table must be 2-D")
        check(_ffi.lib().f110_set_map_dt(self._h, dptr(dt), dt.shape[0], dt.shape[1], float(resolution),
                                         float(origin[0]), float(origin[1]), float(np.cos(origin[2])),
                                         float(np.sin(origin[2]))), self._h)
        self.has_map = True
        self.map_resolution, self.map_origin = float(resolution), list(origin)

    # ---- a different track per env (extension; slot 0 is the map of set_map_*)
    def add_map_image(self, img_top_first, resolution, origin):
        """register another map (same pipeline as set_map_image); returns its slot"""
        img = np.ascontiguousarray(img_top_first, dtype=np.uint8)
        if img.ndim != 2:
            raise ValueError("map image must be 2-D")
        slot = C.c_int32(0)
        check(_ffi.lib().f110_add_map_image(self._h, img.ctypes.data_as(_ffi._u8p), img.shape[0], img.shape[1], float(resolution),
                                            float(origin[0]), float(origin[1]), float(origin[2]), C.byref(slot)), self._h)
        return int(slot.value)

    def add_map_dt(self, dt, resolution, origin):
        dt = as_f64(dt)
        if dt.ndim != 2:
            raise ValueError("distance table must be 2-D")
        slot = C.c_int32(0)
        check(_ffi.lib().f110_add_map_dt(self._h, dptr(dt), dt.shape[0], dt.shape[1], float(resolution), float(origin[0]),
                                         float(origin[1]), float(np.cos(origin[2])), float(np.sin(origin[2])), C.byref(slot)), self._h)
        return int(slot.value)

    def set_env_maps(self, env_map):
        """env_map [num_envs] of slots (None: every env back on slot 0)"""
        if env_map is None:
            check(_ffi.lib().f110_set_env_maps(self._h, None), self._h)
            return
        m = np.ascontiguousarray(env_map, dtype=np.int32).reshape(-1)
        if m.shape[0] != self.E:
            raise ValueError("env_map must have num_envs=%d entries (got %d)" % (self.E, m.shape[0]))
        check(_ffi.lib().f110_set_env_maps(self._h, m.ctypes.data_as(_ffi._i32p)), self._h)

    def get_map_dt(self, slot=0):
        """the distance table of a map slot, row-major [height][width] (row 0 = bottom of the picture)"""
        h, w = C.c_int32(), C.c_int32()
        check(_ffi.lib().f110_slot_shape(self._h, int(slot), C.byref(h), C.byref(w)), self._h)
        out = np.empty((h.value, w.value))
        check(_ffi.lib().f110_get_slot_dt(self._h, int(slot), dptr(out)), self._h)
        return out

    # ---- static obstacles in a derived map slot (extension)
    def add_obstacle_map(self, obstacles, base=0):
        """register a map slot DERIVED from slot `base` (slot 0 or one of add_map_*) with `obstacles` (an Obstacles; None: a copy of
        the base) stamped into its distance table on the device; returns its slot (set_env_maps).  The base's Track, if it has
        one, is attached to the new slot too.  Obstacles are per slot: one padded table of device memory each."""
        from .obstacles import Obstacles
        ob = Obstacles.coerce(obstacles)
        slot = C.c_int32(0)
        check(_ffi.lib().f110_add_map_obstacles(self._h, int(base), ob.structs(), len(ob), C.byref(slot)), self._h)
        t = getattr(self, "tracks", {}).get(int(base))
        if t is not None:
            self.set_track(t, slot=int(slot.value))
        return int(slot.value)

    def set_obstacles(self, slot, obstacles):
        """re-stamp a derived slot in place, from its base: ordered behind the steps in flight and in front of the next one"""
        from .obstacles import Obstacles
        ob = Obstacles.coerce(obstacles)
        check(_ffi.lib().f110_set_map_obstacles(self._h, int(slot), ob.structs(), len(ob)), self._h)

    # ---- a corridor carved into a map slot (extension)
    @staticmethod
    def _corridor_args(tm):
        from .trackgen import TrackMap
        tm = TrackMap.coerce(tm)
        xy, hw = tm.points(), np.ascontiguousarray(tm.widths(), dtype=np.float64)
        return tm, xy, hw, (dptr(xy), dptr(hw), int(xy.shape[0]), int(tm.track.closed))

    def add_track_map(self, tm):
        """register a BASE map slot whose distance table is the corridor of `tm` (a TrackMap; a Track or a dict of random_track's
        arguments are coerced), carved on the device in tm's frame; the line becomes the slot's track.  Returns the slot
        (set_env_maps); obstacle slots may be derived from it."""
        tm, xy, hw, line = self._corridor_args(tm)
        slot = C.c_int32(0)
        check(_ffi.lib().f110_add_map_corridor(self._h, *line, tm.shape[0], tm.shape[1], tm.resolution, tm.origin[0], tm.origin[1], tm.origin[2],
                                               C.byref(slot)), self._h)
        self.track_maps = dict(getattr(self, "track_maps", {}))
        self.track_maps[int(slot.value)] = tm
        self.set_track(tm.track, slot=int(slot.value))
        return int(slot.value)

    def set_track_map(self, slot, tm):
        """re-carve a slot of add_track_map in place with another TrackMap of the same frame (ValueError otherwise) and make its line
        the slot's track: ordered behind the steps in flight and in front of the next one.  Obstacle slots derived from it keep
        their old contents until set_obstacles re-stamps them."""
        tm, xy, hw, line = self._corridor_args(tm)
        old = getattr(self, "track_maps", {}).get(int(slot))
        if old is not None and not old.same_frame(tm):
            raise ValueError("set_track_map: slot %d was carved in the frame %r x %r at %g m, the new map has %r x %r at %g m"
                             % (int(slot), old.shape, old.origin, old.resolution, tm.shape, tm.origin, tm.resolution))
        check(_ffi.lib().f110_set_map_corridor(self._h, int(slot), *line), self._h)
        self.track_maps = dict(getattr(self, "track_maps", {}))
        self.track_maps[int(slot)] = tm
        self.set_track(tm.track, slot=int(slot))

    def corridor_mask(self, tm):
        """f110_corridor_mask_batch (unit form): the carved mask of `tm` uint8 [H][W] (row 0 = bottom, 1 = carved, the border ring 0)
        and the number of carved cells"""
        tm, xy, hw, line = self._corridor_args(tm)
        mask, carved = np.zeros(tm.shape, dtype=np.uint8), np.zeros(1, dtype=np.int64)
        check(_ffi.lib().f110_corridor_mask_batch(self._h, *line, tm.shape[0], tm.shape[1], *tm.frame(), mask.ctypes.data_as(_ffi._u8p),
                                                  carved.ctypes.data_as(_ffi._i64p)), self._h)
        return mask, int(carved[0])

    def corridor_times(self):
        """f110_map_corridor_times: {'mask', 'edt'} in ms of the last add_track_map / set_track_map, by HIP events: the mask kernel
        alone and the two passes of the distance transform"""
        ms = np.zeros(2)
        check(_ffi.lib().f110_map_corridor_times(self._h, dptr(ms)), self._h)
        return dict(mask=float(ms[0]), edt=float(ms[1]))

    # ---- a slot's centreline loop, extracted on the device (extension)
    def slot_frame(self, slot=0):
        """(res, ox, oy, oc, os) of a map slot as the library holds them"""
        out = np.empty(5)
        check(_ffi.lib().f110_slot_frame(self._h, int(slot), dptr(out)), self._h)
        return tuple(float(v) for v in out)

    def centerline_cells(self, slot=0, seed=(0.0, 0.0), heading=None, max_passes=None):
        """f110_map_centerline: the slot's centreline loop as ordered table cells int32 [n][2] (r, c), T at each [n] (the half
        width, metres) and the cells the three stages deleted int64 [3].  The seed is a world point on the track's free region;
        heading (rad) picks the direction of travel, None means counter-clockwise.  Refusals raise ValueError (arguments, the
        seed) or F110LibraryError (no loop, not a simple loop, not converged within max_passes)."""
        h, w = C.c_int32(), C.c_int32()
        check(_ffi.lib().f110_slot_shape(self._h, int(slot), C.byref(h), C.byref(w)), self._h)
        cap = 2 * (int(h.value) + int(w.value)) + 64
        deleted = np.zeros(3, dtype=np.int64)
        n = C.c_int32(0)
        for _ in range(2):   # a second call only when the first guess of the loop's length was too small: n says how much it takes
            cells, hw = np.empty((cap, 2), dtype=np.int32), np.empty(cap)
            rc = _ffi.lib().f110_map_centerline(self._h, int(slot), float(seed[0]), float(seed[1]), int(heading is not None),
                                                0.0 if heading is None else float(heading), 0 if max_passes is None else int(max_passes),
                                                _ffi.i32ptr(cells), dptr(hw), cap, C.byref(n), deleted.ctypes.data_as(_ffi._i64p))
            if rc == _ffi.ERR_INVALID and n.value > cap:
                cap = int(n.value)
                continue
            break
        check(rc, self._h)
        return cells[:n.value].copy(), hw[:n.value].copy(), deleted

    def map_skeleton(self, slot=0, max_passes=None):
        """f110_map_skeleton (debug): the final mask of the thinning rule uint8 [H][W] (row 0 = bottom) and the three totals"""
        h, w = C.c_int32(), C.c_int32()
        check(_ffi.lib().f110_slot_shape(self._h, int(slot), C.byref(h), C.byref(w)), self._h)
        mask, deleted = np.empty((h.value, w.value), dtype=np.uint8), np.zeros(3, dtype=np.int64)
        check(_ffi.lib().f110_map_skeleton(self._h, int(slot), 0 if max_passes is None else int(max_passes), mask.ctypes.data_as(_ffi._u8p),
                                           deleted.ctypes.data_as(_ffi._i64p)), self._h)
        return mask, deleted

    def centerline_times(self):
        """f110_map_centerline_times: {stage: ms} of the last centerline_cells / map_skeleton call, by the host's clock"""
        ms = np.zeros(5)
        check(_ffi.lib().f110_map_centerline_times(self._h, dptr(ms)), self._h)
        return dict(thinning=float(ms[1]), staircase=float(ms[2]), pruning=float(ms[3]), host=float(ms[4]))

    def centerline(self, slot=0, seed=(0.0, 0.0), heading=None, spacing=0.2, smooth=1.0, max_passes=None, return_cells=False):
        """the slot's centreline as a closed Track with the attribute columns half_width and kappa: the loop of cells from the
        device (centerline_cells), then smoothed over `smooth` metres of arc and resampled every `spacing` metres on the host
        (f1tenth_gym_amd/centerline.py states the steps).  return_cells: -> (track, cells, half_width at the cells, deleted)."""
        from .centerline import track_from_cells
        cells, hw, deleted = self.centerline_cells(slot, seed, heading, max_passes)
        track = track_from_cells(cells, hw, self.slot_frame(slot), spacing=spacing, smooth=smooth)
        return (track, cells, hw, deleted) if return_cells else track

    # ---- a racing line and a speed profile per closed track, solved on the device (extension)
    def raceline_batch(self, lines, spec=None, line_iters=None):
        """f110_raceline_batch (unit form): lines [(q [M][2], w [M]), ...] at the settings `spec` (a Raceline, a dict or None; its
        spacing plays no part here), line_iters [T] or None -> (alpha, xy, kappa, vx) with the lines' rows one after the other,
        length [T], lap_time [T]"""
        from .raceline import Raceline
        sp = Raceline.coerce(spec)
        qs = [np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 2) for q, _ in lines]
        ws = [np.ascontiguousarray(w, dtype=np.float64).reshape(-1) for _, w in lines]
        if not lines or any(q.shape[0] != w.shape[0] for q, w in zip(qs, ws)):
            raise ValueError("raceline: at least one line, each with one half width per point")
        T = len(lines)
        off = np.zeros(T + 1, dtype=np.int32)
        off[1:] = np.cumsum([q.shape[0] for q in qs])
        n = int(off[-1])
        xy, hw, beta = np.concatenate(qs), np.concatenate(ws), sp.momentum()
        li = None if line_iters is None else np.ascontiguousarray(line_iters, dtype=np.int32).reshape(T)
        alpha, out_xy, kappa, vx, length, lap = np.zeros(n), np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros(T), np.zeros(T)
        check(_ffi.lib().f110_raceline_batch(self._h, dptr(xy), dptr(hw), i32ptr(off), T, sp.levels, sp.iters, sp.margin, sp.v_max, sp.a_lat, sp.a_accel,
                                             sp.a_brake, dptr(beta) if sp.iters else None, None if li is None else i32ptr(li), dptr(alpha), dptr(out_xy),
                                             dptr(kappa), dptr(vx), dptr(length), dptr(lap)), self._h)
        return alpha, out_xy, kappa, vx, length, lap

    def raceline(self, tracks, spec=None):
        """the raceline of closed tracks that carry a 'half_width' column: `tracks` is a Track, a slot number (that slot's track; on a
        slot of add_track_map that runs on its generating line, the line with the half widths it was carved with) or a list of either; spec a Raceline, a dict of its settings or None.  One device call for the whole list (a workgroup per line,
        and one more per line for the same speed profile on the centreline).  Returns closed Tracks (one for one input) with the
        attribute columns kappa, vx and offset (metres to the left of the centreline) and the attributes lap_time [s], center (the
        stations as a Track with half_width, kappa, vx) and center_lap_time."""
        from .raceline import Raceline, assemble
        from .track import Track
        sp = Raceline.coerce(spec)
        single = isinstance(tracks, Track) or is_int(tracks)
        items = [tracks] if single else list(tracks)
        src = []
        for it in items:
            if is_int(it):
                if int(it) not in getattr(self, "tracks", {}):
                    raise ValueError("raceline: map slot %d has no track (set_track, add_track_map or centerline make one)" % int(it))
                tm = getattr(self, "track_maps", {}).get(int(it))
                # a carved slot that still runs on its generating line: the half widths it was carved with, not the line's column
                it = tm.carved_line() if tm is not None and self.tracks[int(it)] is tm.track and tm.track.closed else self.tracks[int(it)]
            src.append(sp.stations(it))
        lines, iters = [], []
        for q, w in src:            # the line, then the same stations with no iteration: the centreline's own profile
            lines += [(q, w), (q, w)]
            iters += [sp.iters, 0]
        out = self.raceline_batch(lines, sp, iters)
        res = assemble(sp, src, out)
        return res[0] if single else res

    def map_table_address(self, slot=0):
        """(device address of the slot's table cell [0][0], its row pitch in bytes): what the kernels read"""
        p, rb = C.c_void_p(), C.c_int32()
        check(_ffi.lib().f110_slot_table(self._h, int(slot), C.byref(p), C.byref(rb)), self._h)
        return int(p.value or 0), int(rb.value)

    def set_beam_tables(self, scan_angles, cosines, side_distances):
        """replace the per-beam tables of check_ttc_jit / ray_cast (base_classes.py:125-158) — normally built from `params` at creation"""
        sa, co, sd = as_f64(scan_angles, (self.B,)), as_f64(cosines, (self.B,)), as_f64(side_distances, (self.B,))
        check(_ffi.lib().f110_set_beam_tables(self._h, dptr(sa), dptr(co), dptr(sd), self.B), self._h)
        self.scan_angles, self.cosines, self.side_distances = sa, co, sd

    def set_params(self, params, agent_idx=-1):
        pv = _ffi.params_vector(params)
        check(_ffi.lib().f110_set_params(self._h, int(agent_idx), dptr(pv)), self._h, IndexError)
        self._slot_rows[slice(None) if int(agent_idx) < 0 else int(agent_idx)] = pv

    def agent_params_rows(self):
        """[A][18] float64: the agent slots' parameter sets (the constructor's, then set_params'): a parameter sampler's nominal rows"""
        return self._slot_rows.copy()

    def set_params_batch(self, params):
        """one vehicle parameter set per agent: a list of N dicts or an [N][18] array in PARAM_KEYS
        order; None returns to the per-slot sets of set_params"""
        if params is None:
            check(_ffi.lib().f110_set_params_batch(self._h, None), self._h)
            return
        if isinstance(params, (list, tuple)) and len(params) and isinstance(params[0], dict):
            params = np.stack([_ffi.params_vector(p) for p in params])
        pv = as_f64(params)
        if pv.shape != (self.N, len(_ffi.PARAM_KEYS)):
            raise ValueError("per-agent parameters must be [num_envs*num_agents][%d]" % len(_ffi.PARAM_KEYS))
        check(_ffi.lib().f110_set_params_batch(self._h, dptr(pv)), self._h)

    def set_noise_table(self, noise):
        if noise is None:
            check(_ffi.lib().f110_set_noise_table(self._h, None, 0, self.B), self._h)
            self.noise_rows = 0
            return
        noise = as_f64(noise)
        if noise.ndim != 2 or noise.shape[1] != self.B:
            raise ValueError("noise table must be [rows][num_beams]")
        check(_ffi.lib().f110_set_noise_table(self._h, dptr(noise), noise.shape[0], self.B), self._h)
        self.noise_rows = noise.shape[0]

    # ---- scan noise generated on the device: np.random.default_rng(seed).normal(0, std, B) per scan
    @staticmethod
    def pcg64_state(seed):
        """(state.hi, state.lo, inc.hi, inc.lo) of np.random.PCG64(seed), computed by the library's
        restatement of SeedSequence + pcg64_set_seed (seed: int in [0, 2^64))"""
        out = (C.c_uint64 * 4)()
        check(_ffi.lib().f110_pcg64_seed(C.c_uint64(int(seed)), out), None)
        return np.array(list(out), dtype=np.uint64)

    @staticmethod
    def _state_words(seed):
        """any seed NumPy accepts (None, int of any size, sequence, SeedSequence) -> the 4 state words"""
        if isinstance(seed, (int, np.integer)) and 0 <= int(seed) < 2 ** 64:
            return BatchSim.pcg64_state(seed)
        st = np.random.PCG64(seed).state['state']
        m = (1 << 64) - 1
        return np.array([st['state'] >> 64, st['state'] & m, st['inc'] >> 64, st['inc'] & m], dtype=np.uint64)

    def set_noise_rng(self, seed, std_dev=0.01, per_agent_seeds=None, cache_rows=0, enabled=True):
        """the reference's scan noise (laser_models.py:450-452, base_classes.py:204) drawn on the
        device, bit-identical to NumPy's stream.  seed: every agent's stream (as in the reference) —
        anything np.random.default_rng accepts, None included (fresh OS entropy, exactly as
        default_rng(None) in the reference); per_agent_seeds [N]: a stream per agent instead (extension).
        enabled=False (or set_noise_off()) switches the noise off; a seed never does."""
        L = _ffi.lib()
        if not enabled:
            check(L.f110_set_noise_rng(self._h, None, 0, 0.0, 0), self._h)
        elif per_agent_seeds is not None:
            seeds = list(per_agent_seeds)
            if len(seeds) != self.N:
                raise ValueError("per_agent_seeds must have num_envs*num_agents=%d entries" % self.N)
            words = np.ascontiguousarray(np.stack([self._state_words(s) for s in seeds]), dtype=np.uint64)
            check(L.f110_set_noise_rng(self._h, words.ctypes.data_as(_ffi._u64p), 1, float(std_dev), 0), self._h)
        else:
            words = np.ascontiguousarray(self._state_words(seed), dtype=np.uint64)
            check(L.f110_set_noise_rng(self._h, words.ctypes.data_as(_ffi._u64p), 0, float(std_dev), int(cache_rows)), self._h)
        self.noise_rows = 0

    def set_noise_off(self):
        self.set_noise_rng(None, enabled=False)

    def noise_prepare(self, rows):
        check(_ffi.lib().f110_noise_prepare(self._h, int(rows)), self._h)

    def noise_rows_batch(self, seed, rows, num_beams=None, std_dev=0.01):
        """unit entry point: `rows` consecutive rng.normal(0, std_dev, num_beams) draws of
        default_rng(seed) -> (array [rows][num_beams], generator state after them as a Python int)"""
        B = self.B if num_beams is None else int(num_beams)
        words = np.ascontiguousarray(self._state_words(seed), dtype=np.uint64)
        out = np.empty((int(rows), B))
        st = (C.c_uint64 * 2)()
        check(_ffi.lib().f110_noise_rows_batch(self._h, words.ctypes.data_as(_ffi._u64p), float(std_dev), int(rows), B, dptr(out), st), self._h)
        return out, (int(st[0]) << 64) | int(st[1])

    def scan_lookup_count(self, enable=None, read=True, detail=False):
        """measurement aid: table lookups of every ray the step's scan kernels marched since the last read
        (detail=True: also how many of them the LDS window of map_layout 4 served)"""
        v = (C.c_int64 * 2)()
        check(_ffi.lib().f110_scan_lookup_count(self._h, -1 if enable is None else int(bool(enable)), v if read else None), self._h)
        return (int(v[0]), int(v[1])) if detail else int(v[0])

    # ------------------------------------------------------------------ reset / step
    def reset(self, poses, env_mask=None):
        poses = as_f64(poses)
        if poses.shape[0] != self.N:
            raise ValueError('Number of poses for reset does not match number of agents.')  # base_classes.py:625
        poses = as_f64(poses, (self.N, 3))
        mptr = None
        if env_mask is not None:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            if m.shape != (self.E,):
                raise ValueError("env_mask must have num_envs entries")
            mptr = m.ctypes.data_as(_ffi._u8p)
        check(_ffi.lib().f110_reset(self._h, dptr(poses), mptr), self._h)

    def step(self, actions):
        actions = as_f64(actions, (self.N, 2))
        check(_ffi.lib().f110_step(self._h, dptr(actions)), self._h)

    def step_device(self, d_actions):
        ptr = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_step_device(self._h, ptr), self._h)

    def reset_device(self, d_poses, d_mask=None):
        p = d_poses.ptr if isinstance(d_poses, DeviceArray) else int(d_poses)
        m = None if d_mask is None else (d_mask.ptr if isinstance(d_mask, DeviceArray) else int(d_mask))
        check(_ffi.lib().f110_reset_device(self._h, p, m), self._h)

    def reset_collided_device(self, d_start_poses, ego_idx=0, d_count=None):
        """device-side mask reset of every env whose ego has collided (no host sync)"""
        p = d_start_poses.ptr if isinstance(d_start_poses, DeviceArray) else int(d_start_poses)
        c = None if d_count is None else (d_count.ptr if isinstance(d_count, DeviceArray) else int(d_count))
        check(_ffi.lib().f110_reset_collided_device(self._h, p, int(ego_idx), c), self._h, IndexError)

    def set_auto_reseat(self, d_start_poses, ego_idx=0, d_count=None):
        """fold reset_collided_device into the end of every following step (None disarms it)"""
        p = None if d_start_poses is None else (d_start_poses.ptr if isinstance(d_start_poses, DeviceArray) else int(d_start_poses))
        c = None if d_count is None else (d_count.ptr if isinstance(d_count, DeviceArray) else int(d_count))
        check(_ffi.lib().f110_set_auto_reseat(self._h, p, int(ego_idx), c), self._h, IndexError)
        self._reseat_refs = (d_start_poses, d_count)   # keep the device buffers alive while armed

    # ------------------------------------------------------------------ optional RCCL observation gather
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        check(_ffi.lib().f110_comm_unique_id(buf), None)
        return buf.raw

    def comm_init(self, n_ranks, rank, unique_id):
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(_ffi.lib().f110_comm_init(self._h, int(n_ranks), int(rank), buf), self._h)
        self.comm_ranks = int(n_ranks)

    def comm_set_overlap(self, enable=True):
        """double-buffer the scans so that comm_all_gather_scans overlaps the following step"""
        check(_ffi.lib().f110_comm_set_overlap(self._h, 1 if enable else 0), self._h)

    def comm_all_gather_scans(self, d_recv):
        ptr = d_recv.ptr if isinstance(d_recv, DeviceArray) else int(d_recv)
        check(_ffi.lib().f110_comm_all_gather_scans(self._h, ptr), self._h)

    OBS_SCALARS = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "linear_vels_y", "ang_vels_z", "collisions")

    def comm_all_gather_obs(self, d_recv_scans, d_recv_scalars):
        """the whole observation to every rank: scans [ranks][N][B] and the scalar block
        [ranks][7][N] in OBS_SCALARS order (one RCCL group, see f110_comm_all_gather_obs)"""
        a = d_recv_scans.ptr if isinstance(d_recv_scans, DeviceArray) else int(d_recv_scans)
        b = d_recv_scalars.ptr if isinstance(d_recv_scalars, DeviceArray) else int(d_recv_scalars)
        check(_ffi.lib().f110_comm_all_gather_obs(self._h, a, b), self._h)

    def comm_gather_obs(self, d_recv_scans, d_recv_scalars, f32=False, root=None):
        """f110_comm_gather_obs: the observation gather with float32 transport of the scans (d_recv_scans then holds
        float32 [ranks][N][B]) and / or to ONE receiving rank (root; None: every rank, the all-gather)"""
        def ptr(x):
            return None if x is None else (x.ptr if isinstance(x, DeviceArray) else int(x))
        check(_ffi.lib().f110_comm_gather_obs(self._h, ptr(d_recv_scans), ptr(d_recv_scalars), _ffi.GATHER_F32 if f32 else _ffi.GATHER_F64,
                                              -1 if root is None else int(root)), self._h)

    def step_groups(self):
        """(env blocks the handle can submit a step as, candidate streams probed at creation, blocks of the most recent
        step_device) — f110_step_groups"""
        g, p, l = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(_ffi.lib().f110_step_groups(self._h, C.byref(g), C.byref(p), C.byref(l)), self._h)
        return int(g.value), int(p.value), int(l.value)

    def step_launches(self):
        """1 when the most recent step ran as ONE kernel launch (k_step_tiny: at most 4 agents, one or two per env), else 0"""
        n = C.c_int32(0)
        check(_ffi.lib().f110_step_launches(self._h, C.byref(n)), self._h)
        return int(n.value)

    def comm_info(self):
        """(n_ranks, rank) as RCCL reports them"""
        n, r = C.c_int32(0), C.c_int32(-1)
        check(_ffi.lib().f110_comm_info(self._h, C.byref(n), C.byref(r)), self._h)
        return int(n.value), int(r.value)

    # ------------------------------------------------------------------ episode logic on the device
    def episode_init(self, ego_idx=0):
        check(_ffi.lib().f110_episode_init(self._h, int(ego_idx)), self._h, IndexError)
        self._ep_ego = int(ego_idx)

    def episode_reset(self, poses, env_mask=None):
        """F110Env.reset's state part (f110_env.py:319-334) for the masked envs: lap bookkeeping
        cleared, start poses + start_rot stored, simulator state reset."""
        poses = as_f64(poses, (self.N, 3))
        th = -poses.reshape(self.E, self.A, 3)[:, self._ep_ego, 2]
        rot = np.stack([np.cos(th), -np.sin(th), np.sin(th), np.cos(th)], axis=1)   # start_rot :331
        rot = np.ascontiguousarray(rot, dtype=np.float64)
        mptr = None
        if env_mask is not None:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            mptr = m.ctypes.data_as(_ffi._u8p)
        check(_ffi.lib().f110_episode_reset(self._h, dptr(poses), dptr(rot), mptr), self._h)

    _ep_ego = 0

    def episode_step_device(self, d_actions):
        ptr = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_episode_step_device(self._h, ptr), self._h)

    def episode_reset_done_device(self, d_count=None):
        c = None if d_count is None else (d_count.ptr if isinstance(d_count, DeviceArray) else int(d_count))
        check(_ffi.lib().f110_episode_reset_done_device(self._h, c), self._h)

    def pinned_empty(self, shape, dtype=np.float64):
        """a NumPy array over page-locked host memory (full-rate DMA).  The memory lives as long as any
        array that views it (slices, .view(), reshape ...) and is returned when the last one is collected —
        closing the BatchSim first is fine."""
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(_ffi.lib().f110_host_alloc(self._h, nbytes, C.byref(p)), self._h)
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)   # every NumPy view keeps `buf` alive through .base
        weakref.finalize(buf, _ffi.lib().f110_host_free, None, p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    # ------------------------------------------------------------------ one call per env.step()
    HOST_FIELDS = {   # name -> (dtype, shape as a function of (N, E, B))
        "state": (np.float64, lambda N, E, B: (7, N)), "collisions": (np.float64, lambda N, E, B: (N,)),
        "collision_idx": (np.float64, lambda N, E, B: (N,)), "agent_poses": (np.float64, lambda N, E, B: (3, N)),
        "lap_times": (np.float64, lambda N, E, B: (N,)), "lap_counts": (np.float64, lambda N, E, B: (N,)),
        "toggles": (np.float64, lambda N, E, B: (N,)), "current_time": (np.float64, lambda N, E, B: (E,)),
        "in_collision": (np.int32, lambda N, E, B: (N,)), "near_starts": (np.uint8, lambda N, E, B: (N,)),
        "checkpoint_done": (np.uint8, lambda N, E, B: (N,)), "done": (np.uint8, lambda N, E, B: (E,)),
        "scans": (np.float64, lambda N, E, B: (N, B))}

    def host_block(self, fields):
        """page-locked memory for f110_step_host: returns an object with .actions ([N][2], written by the
        caller), one NumPy view per requested field (attribute .views, a dict) and the ctypes struct.
        The views are OVERWRITTEN by every step_host(): copy what you keep."""
        fields = tuple(fields)
        for f in fields:
            if f not in self.HOST_FIELDS:
                raise KeyError(f)
        N, E, B = self.N, self.E, self.B
        offs, total = {}, 16 * N     # the actions lead the block
        for f in fields:
            dt, shp = self.HOST_FIELDS[f]
            total = (total + 255) // 256 * 256
            offs[f] = total
            total += int(np.prod(shp(N, E, B))) * np.dtype(dt).itemsize
        raw = self.pinned_empty((total,), np.uint8)
        hb = types.SimpleNamespace(raw=raw, fields=fields, views={}, struct=_ffi.HostBlock())
        hb.actions = raw[:16 * N].view(np.float64).reshape(N, 2)
        hb.actions[...] = 0.0
        for f in fields:
            dt, shp = self.HOST_FIELDS[f]
            shape = shp(N, E, B)
            nb = int(np.prod(shape)) * np.dtype(dt).itemsize
            v = raw[offs[f]:offs[f] + nb].view(dt).reshape(shape)
            hb.views[f] = v
            setattr(hb.struct, f, v.ctypes.data_as(dict(_ffi.HostBlock._fields_)[f]))
        hb.struct_ref = C.byref(hb.struct)
        hb.actions_ptr = hb.actions.ctypes.data
        return hb

    def step_host_stats(self):
        """(calls, mean host us enqueuing, mean host us waiting) of step_host since the last read"""
        o = np.zeros(3)
        check(_ffi.lib().f110_step_host_stats(self._h, dptr(o)), self._h)
        n = max(o[0], 1.0)
        return int(o[0]), o[1] / n, o[2] / n

    def step_host(self, hb, actions=None, auto_reset=False, sync=True, mapped_actions=True, spin=False, fuse=True, poll=True, scripted=False):
        """f110_step_host: `actions` (None: hb.actions as the caller filled it in place) up, the step, the
        episode logic if episode_init was called, hb's fields down — one ABI call.  scripted: the armed controllers
        (set_controllers) replace their agents' rows on the device before the step."""
        flags = (_ffi.STEP_AUTO_RESET if auto_reset else 0) | (0 if sync else _ffi.STEP_NO_SYNC) | (_ffi.STEP_SPIN_WAIT if spin else 0)
        if scripted:
            flags |= _ffi.STEP_SCRIPTED
        if not fuse:
            flags |= _ffi.STEP_NO_FUSE
        if poll:
            flags |= _ffi.STEP_POLL
        if actions is None or actions is hb.actions:
            ptr = hb.actions_ptr
            if mapped_actions:
                flags |= _ffi.STEP_ACTIONS_MAPPED
        else:
            a = as_f64(actions, (self.N, 2))
            ptr = a.ctypes.data
        rc = _ffi.lib().f110_step_host(self._h, ptr, hb.struct_ref, flags)
        if rc:
            check(rc, self._h)

    def step_host_inplace(self, hb):
        """step_host(hb) with its defaults (the actions as the caller left them in hb.actions, read in place; wait by polling), without
        the argument handling: the single-env loop counts microseconds"""
        rc = self._f_step_host(self._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_POLL | _ffi.STEP_ACTIONS_MAPPED)
        if rc:
            check(rc, self._h)

    def episode_step_host(self, actions_pinned, packed_pinned, auto_reset=False):
        """actions up, step, _check_done, the packed scalar observation down (one copy), optional re-seat;
        returns views into packed_pinned (overwritten by the next call)"""
        check(_ffi.lib().f110_episode_step_host(self._h, actions_pinned.ctypes.data, 1 if auto_reset else 0, packed_pinned.ctypes.data), self._h)
        N, E = self.N, self.E
        cols = packed_pinned[:(9 * N + E) * 8].view(np.float64)
        fl = packed_pinned[(9 * N + E) * 8:]
        names = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions", "lap_times", "lap_counts", "toggles")
        out = {k: cols[i * N:(i + 1) * N] for i, k in enumerate(names)}
        out["current_time"] = cols[9 * N:9 * N + E]
        out["near_starts"], out["checkpoint_done"], out["done"] = fl[:N], fl[N:2 * N], fl[2 * N:2 * N + E]
        return out

    def packed_bytes(self):
        return int(_ffi.lib().f110_episode_packed_bytes(self._h))

    def episode_get(self):
        N, E = self.N, self.E
        out = {"lap_times": np.empty(N), "lap_counts": np.empty(N), "toggles": np.empty(N),
               "current_time": np.empty(E), "near_starts": np.empty(N, dtype=np.uint8),
               "done": np.empty(E, dtype=np.uint8), "checkpoint_done": np.empty(N, dtype=np.uint8)}
        o = _ffi.EpisodeHost()
        for k in ("lap_times", "lap_counts", "toggles", "current_time"):
            setattr(o, k, dptr(out[k]))
        for k in ("near_starts", "done", "checkpoint_done"):
            setattr(o, k, out[k].ctypes.data_as(_ffi._u8p))
        check(_ffi.lib().f110_episode_get(self._h, C.byref(o)), self._h)
        return out

    def episode_device_views(self):
        v = _ffi.EpisodeViews()
        check(_ffi.lib().f110_episode_device_views(self._h, C.byref(v)), self._h)
        sp, sr = C.c_void_p(), C.c_void_p()
        check(_ffi.lib().f110_episode_start_views(self._h, C.byref(sp), C.byref(sr)), self._h)
        N, E = self.N, self.E
        return {"done": DeviceArray(self, (E,), np.uint8, v.done),
                "checkpoint_done": DeviceArray(self, (N,), np.uint8, v.checkpoint_done),
                "lap_times": DeviceArray(self, (N,), np.float64, v.lap_times),
                "lap_counts": DeviceArray(self, (N,), np.float64, v.lap_counts),
                "toggles": DeviceArray(self, (N,), np.float64, v.toggles),
                "current_time": DeviceArray(self, (E,), np.float64, v.current_time),
                "start_poses": DeviceArray(self, (N, 3), np.float64, sp.value), "start_rot": DeviceArray(self, (E, 4), np.float64, sr.value)}

    def device_mem_info(self):
        """(free, total) bytes of the handle's GPU"""
        f, t = C.c_size_t(0), C.c_size_t(0)
        check(_ffi.lib().f110_device_mem_info(self._h, C.byref(f), C.byref(t)), self._h)
        return int(f.value), int(t.value)

    def device_array(self, shape, dtype=np.float64):
        return DeviceArray(self, shape, dtype)

    def device_views(self):
        v = _ffi.DeviceViews()
        check(_ffi.lib().f110_get_device_views(self._h, C.byref(v)), self._h)
        N, B = self.N, self.B
        return {"scans": DeviceArray(self, (N, B), np.float64, v.scans),
                "state": DeviceArray(self, (7, N), np.float64, v.state),
                "agent_poses": DeviceArray(self, (3, N), np.float64, v.agent_poses),
                "collisions": DeviceArray(self, (N,), np.float64, v.collisions),
                "collision_idx": DeviceArray(self, (N,), np.float64, v.collision_idx),
                "in_collision": DeviceArray(self, (N,), np.int32, v.in_collision),
                "step_count": DeviceArray(self, (N,), np.int32, v.step_count),
                "stream": v.stream}

    _F64 = ("scans", "poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions",
            "collision_idx", "state", "agent_poses")
    _I32 = ("in_collision", "step_count")

    def get(self, *fields):
        """Read back (and synchronise).  fields from: scans poses_x poses_y poses_theta
        linear_vels_x ang_vels_z collisions collision_idx state agent_poses in_collision step_count."""
        N, B = self.N, self.B
        shapes = {"scans": (N, B), "state": (N, 7), "agent_poses": (N, 3)}
        o = _ffi.ObsHost()
        out = {}
        for f in fields:
            if f in self._F64:
                out[f] = np.empty(shapes.get(f, (N,)), dtype=np.float64)
                setattr(o, f, dptr(out[f]))
            elif f in self._I32:
                out[f] = np.empty((N,), dtype=np.int32)
                setattr(o, f, i32ptr(out[f]))
            else:
                raise KeyError(f)
        check(_ffi.lib().f110_get_obs(self._h, C.byref(o)), self._h)
        return out

    def set_state(self, state, steer_buf=None, buf_count=None):
        """A PARTIAL setter (f110_set_state): RaceCar.state, the steering FIFO and its count only.  step_count, the collision
        flags, agent_poses, noise-stream positions and the episode arrays stay as they are, so a batch "restored" this way
        diverges at its first noisy scan — save_state / load_state restore all of it."""
        state = as_f64(state, (self.N, 7))
        sb = None if steer_buf is None else as_f64(steer_buf, (self.N, 2))
        bc = None if buf_count is None else np.ascontiguousarray(buf_count, dtype=np.int32)
        check(_ffi.lib().f110_set_state(self._h, dptr(state), None if sb is None else dptr(sb),
                                        None if bc is None else i32ptr(bc)), self._h)

    # ------------------------------------------------------------------ exact snapshot / restore / clone (f110_state_*)
    def _state_call(self, rc):
        if rc == _ffi.ERR_STATE:   # a blob that does not fit this handle
            raise ValueError(_ffi.last_error(self._h))
        check(rc, self._h)

    def state_bytes(self, n_envs=None, scans=False):
        """bytes of a blob of n_envs envs (all by default) with this handle's current columns"""
        return int(_ffi.lib().f110_state_bytes(self._h, self.E if n_envs is None else int(n_envs), _ffi.STATE_SCANS if scans else 0))

    def save_state(self, scans=True, out=None):
        """every env's state (and the last scans) -> StateBlob.  out: a uint8 buffer of state_bytes() bytes to fill (pinned_empty
        memory copies at full rate)"""
        flags = _ffi.STATE_SCANS if scans else 0
        n = self.state_bytes(None, scans)
        buf = np.empty(n, dtype=np.uint8) if out is None else out
        if buf.dtype != np.uint8 or buf.ndim != 1 or buf.nbytes != n or not buf.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 buffer of %d bytes" % n)
        self._state_call(_ffi.lib().f110_state_save(self._h, buf.ctypes.data, flags))
        return StateBlob(buf)

    def load_state(self, blob):
        """restore every env from a save_state blob of a handle of the same shape (agents, beams, envs) and configuration"""
        blob = blob if isinstance(blob, StateBlob) else StateBlob(blob)
        self._state_call(_ffi.lib().f110_state_load(self._h, blob.data.ctypes.data))

    def _indices(self, idx, what, limit):
        """(pointer, count, keep-alive) of an index list: a DeviceArray of int32 as it is, host indices checked and uploaded"""
        if isinstance(idx, DeviceArray):
            if idx.dtype != np.int32 or len(idx.shape) != 1:
                raise ValueError("%s: a device index list is a 1-D int32 DeviceArray" % what)
            return idx.ptr, idx.shape[0], idx, None
        a = np.atleast_1d(np.asarray(idx))
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s must be a 1-D list of integer indices" % what)
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= limit):
            raise ValueError("%s: indices must lie in [0, %d), got %s" % (what, limit, a[(a < 0) | (a >= limit)][:8].tolist()))
        a = np.ascontiguousarray(a, dtype=np.int32)
        if a.size == 0:
            return None, 0, None, a
        d = self.device_array((a.size,), np.int32)
        d.upload(a)
        return d.ptr, a.size, d, a

    @staticmethod
    def _status_ptr(d_status):
        return None if d_status is None else (d_status.ptr if isinstance(d_status, DeviceArray) else int(d_status))

    def save_envs(self, env_idx, scans=False, device=False):
        """the state of envs env_idx (host indices or an int32 DeviceArray) -> a StateBlob whose entry j is env env_idx[j], or
        (device=True) a DeviceArray holding the blob, which load_envs takes without a host round trip"""
        ptr, k, keep, _ = self._indices(env_idx, "env_idx", self.E)
        if k == 0:
            raise ValueError("env_idx is empty")
        flags = _ffi.STATE_SCANS if scans else 0
        d_blob = self.device_array((self.state_bytes(k, scans),), np.uint8)
        self._state_call(_ffi.lib().f110_state_save_device(self._h, ptr, k, d_blob.ptr, flags))
        del keep
        if device:
            return d_blob
        blob = StateBlob(d_blob.download())
        d_blob.free()
        return blob

    def load_envs(self, blob, src, dst, d_status=None):
        """blob entry src[j] -> env dst[j] (several dst may share a src).  Host index lists are checked (range, no dst twice:
        ValueError); device lists (int32 DeviceArrays) are not — their out-of-range entries are skipped and counted into the
        device int32 d_status, and a dst named twice is undefined."""
        d_blob, tmp = blob, None
        if not isinstance(blob, DeviceArray):
            blob = blob if isinstance(blob, StateBlob) else StateBlob(blob)
            tmp = d_blob = self.device_array((blob.nbytes,), np.uint8)
            d_blob.upload(blob.data)
            k_blob = blob.num_envs
        else:
            k_blob = None
        sp, ks, skeep, _ = self._indices(src, "src", k_blob if k_blob is not None else 1 << 30)
        dp, kd, dkeep, dh = self._indices(dst, "dst", self.E)
        if ks != kd:
            raise ValueError("src and dst must have the same length (%d != %d)" % (ks, kd))
        if dh is not None and np.unique(dh).size != dh.size:
            raise ValueError("dst names an env more than once")
        if kd:
            self._state_call(_ffi.lib().f110_state_load_device(self._h, d_blob.ptr, sp, dp, kd, self._status_ptr(d_status)))
        del skeep, dkeep
        if tmp is not None:
            tmp.free()

    def clone_envs(self, src, dst, d_status=None):
        """env src[j] -> env dst[j] on the device, one launch (the branching primitive: MCTS, forked rollouts).  Host index
        lists are checked: in range, src and dst disjoint, no dst twice (ValueError); device lists are not (out-of-range entries
        are skipped and counted into d_status)."""
        sp, ks, skeep, sh = self._indices(src, "src", self.E)
        dp, kd, dkeep, dh = self._indices(dst, "dst", self.E)
        if ks != kd:
            raise ValueError("src and dst must have the same length (%d != %d)" % (ks, kd))
        if dh is not None:
            if np.unique(dh).size != dh.size:
                raise ValueError("dst names an env more than once")
            if sh is not None and np.intersect1d(sh, dh).size:
                raise ValueError("src and dst overlap (envs %s): a clone reads and writes disjoint envs" % np.intersect1d(sh, dh)[:8].tolist())
        if kd:
            self._state_call(_ffi.lib().f110_clone_envs_device(self._h, sp, dp, kd, self._status_ptr(d_status)))
        del skeep, dkeep

    # ------------------------------------------------------------------ randomised start poses
    def set_reset_sampler(self, seed, s_range=(0.0, 1.0), gap=1.0, lateral=0.0, heading=0.0, clearance=None, attempts=16,
                          env_base=0):
        """arm the start-pose sampler: every explicit sample_reset and every in-step re-seat then draws the env's start poses on
        its slot's track (f110_reset_sampler_set).  seed: a ResetSampler (its settings win) or anything SeedSequence takes; env
        e draws from PCG64(SeedSequence(seed, spawn_key=(env_base + e,))).  clearance None: half the car's diagonal.
        Returns the ResetSampler."""
        from .reset_sampler import ResetSampler
        rs = seed if isinstance(seed, ResetSampler) else ResetSampler(seed, s_range, gap, lateral, heading, clearance, attempts)
        if int(env_base) < 0:
            raise ValueError("env_base must be >= 0, got %d" % int(env_base))
        words = np.ascontiguousarray(rs.streams(self.E, int(env_base)), dtype=np.uint64)
        spec = rs.spec(float(self.params['length']), float(self.params['width']))
        check(_ffi.lib().f110_reset_sampler_set(self._h, C.byref(spec), words.ctypes.data_as(_ffi._u64p)), self._h)
        self.reset_sampler = rs
        return rs

    def clear_reset_sampler(self):
        check(_ffi.lib().f110_reset_sampler_set(self._h, None, None), self._h)
        self.reset_sampler = None

    reset_sampler = None

    def sample_reset(self, env_mask=None):
        """explicit draw for the envs of env_mask (None: all): f110_reset (and the episode reset) to the drawn poses"""
        mptr, m = None, None
        if env_mask is not None:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            if m.shape != (self.E,):
                raise ValueError("env_mask must have num_envs=%d entries" % self.E)
            mptr = m.ctypes.data_as(_ffi._u8p)
        check(_ffi.lib().f110_reset_sample(self._h, mptr), self._h)

    def sample_reset_device(self, d_mask=None):
        ptr = None if d_mask is None else (d_mask.ptr if isinstance(d_mask, DeviceArray) else int(d_mask))
        check(_ffi.lib().f110_reset_sample_device(self._h, ptr), self._h)

    def reset_sampler_stats(self, clear=False, attempts=False):
        """{'draws', 'fallbacks'} since the last clear; attempts=True adds 'attempt' [E] (winning attempt of each env's last
        draw, -1 = fallback / none)"""
        v = (C.c_uint64 * 2)()
        att = np.empty((self.E,), dtype=np.int32) if attempts else None
        check(_ffi.lib().f110_reset_sampler_stats(self._h, v, None if att is None else att.ctypes.data_as(_ffi._i32p),
                                                  1 if clear else 0), self._h)
        out = {"draws": int(v[0]), "fallbacks": int(v[1])}
        if att is not None:
            out["attempt"] = att
        return out

    def reset_sampler_poses(self):
        """[N][3] poses of each env's last reset of any kind (what an explicit fallback resets to; after a draw: the drawn ones)"""
        out = np.empty((self.N, 3))
        check(_ffi.lib().f110_reset_sampler_poses(self._h, dptr(out)), self._h)
        return out

    # ------------------------------------------------------------------ randomised vehicle parameters
    def set_param_sampler(self, sampler, env_base=0):
        """arm the parameter sampler: every explicit sample_params and every re-seat then draws the env's rows of the per-agent
        parameter block (f110_param_sampler_set); no draw happens here, the rows start as the per-slot sets.  sampler: a
        ParamSampler or a dict of its settings; env e draws from PCG64(SeedSequence(seed, spawn_key=(env_base + e,))), the reset
        sampler's rule: give the two different seeds.  Returns the ParamSampler."""
        from .param_sampler import ParamSampler
        ps = ParamSampler.coerce(sampler)
        ps.validate(self._slot_rows)   # (a ValueError that names the parameter, before any ABI call)
        if int(env_base) < 0:
            raise ValueError("env_base must be >= 0, got %d" % int(env_base))
        words = np.ascontiguousarray(ps.streams(self.E, int(env_base)), dtype=np.uint64)
        entries = ps.entries()
        check(_ffi.lib().f110_param_sampler_set(self._h, entries, words.ctypes.data_as(_ffi._u64p)), self._h)
        self.param_sampler = ps
        return ps

    def clear_param_sampler(self):
        check(_ffi.lib().f110_param_sampler_set(self._h, None, None), self._h)
        self.param_sampler = None

    param_sampler = None

    def sample_params(self, env_mask=None):
        """explicit draw for the envs of env_mask (None: all); nothing is reset"""
        mptr, m = None, None
        if env_mask is not None:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            if m.shape != (self.E,):
                raise ValueError("env_mask must have num_envs=%d entries" % self.E)
            mptr = m.ctypes.data_as(_ffi._u8p)
        check(_ffi.lib().f110_param_sample(self._h, mptr), self._h)

    def sample_params_device(self, d_mask=None):
        ptr = None if d_mask is None else (d_mask.ptr if isinstance(d_mask, DeviceArray) else int(d_mask))
        check(_ffi.lib().f110_param_sample_device(self._h, ptr), self._h)

    def param_sampler_stats(self, clear=False):
        """{'draws'}: envs drawn since the last clear"""
        v = (C.c_uint64 * 1)()
        check(_ffi.lib().f110_param_sampler_stats(self._h, v, 1 if clear else 0), self._h)
        return {"draws": int(v[0])}

    def get_params(self):
        """[N][18] float64: the live per-agent rows (the parameter sampler's or set_params_batch's)"""
        out = np.empty((self.N, _ffi.NPARAMS))
        check(_ffi.lib().f110_params_get(self._h, dptr(out)), self._h)
        return out

    def params_view(self):
        """the live per-agent rows [N][18] as a DeviceArray (no copy; exports through DLPack): what a policy or critic reads as
        privileged input.  The view is the handle's memory: it ends with clear_param_sampler / close."""
        p = C.c_void_p()
        check(_ffi.lib().f110_params_view(self._h, C.byref(p)), self._h)
        return DeviceArray(self, (self.N, _ffi.NPARAMS), np.float64, ptr=p.value)

    def param_sample_rows(self, sampler, nominal, streams, rounds=1, num_agents=None):
        """unit form (f110_param_sample_batch): the envs of `streams` ([m][4] words) drawn `rounds` times over the nominal rows
        [A][18] (or one parameter dict and num_agents).  Returns (rows [rounds][m * A][18], the streams afterwards [m][4])."""
        from .param_sampler import ParamSampler, nominal_rows
        ps = ParamSampler.coerce(sampler)
        nom = nominal_rows(nominal, num_agents)
        words = np.ascontiguousarray(streams, dtype=np.uint64)
        if words.ndim != 2 or words.shape[1] != 4:
            raise ValueError("streams must be [m][4] uint64 words")
        m, A, rounds = int(words.shape[0]), int(nom.shape[0]), int(rounds)
        out = np.empty((max(rounds, 0), m * A, _ffi.NPARAMS))
        after = np.empty_like(words)
        check(_ffi.lib().f110_param_sample_batch(self._h, ps.entries(), dptr(nom), A, words.ctypes.data_as(_ffi._u64p), m, rounds, dptr(out),
                                                 after.ctypes.data_as(_ffi._u64p)), self._h)
        return out, after

    # ------------------------------------------------------------------ timing (bench.py)
    def timer_begin(self):
        check(_ffi.lib().f110_timer_begin(self._h), self._h)

    def timer_end_ms(self):
        ms = C.c_double()
        check(_ffi.lib().f110_timer_end_ms(self._h, C.byref(ms)), self._h)
        return ms.value

    def profile_kernels(self, enable):
        check(_ffi.lib().f110_profile_kernels(self._h, 1 if enable else 0), self._h)

    def profile_read(self):
        n = C.c_int32(); s = C.c_double(); d = C.c_double(); f = C.c_double()
        check(_ffi.lib().f110_profile_read(self._h, C.byref(n), C.byref(s), C.byref(d), C.byref(f)), self._h)
        return n.value, s.value, d.value, f.value

    # ------------------------------------------------------------------ unit entry points
    def scan_batch(self, poses, want_hits=False, want_lookups=False):
        poses = as_f64(poses)
        if poses.ndim != 2 or poses.shape[1] != 3:
            raise ValueError("poses must be [M][3]")
        m = poses.shape[0]
        ranges = np.empty((m, self.B))
        hits = np.empty((m, self.B, 2), dtype=np.int32) if want_hits else None
        lk = np.zeros((m,), dtype=np.int64) if want_lookups else None
        check(_ffi.lib().f110_scan_batch(self._h, dptr(poses), m, dptr(ranges),
                                         None if hits is None else i32ptr(hits),
                                         None if lk is None else lk.ctypes.data_as(_ffi._i64p)), self._h)
        res = [ranges]
        if want_hits:
            res.append(hits)
        if want_lookups:
            res.append(lk)
        return res[0] if len(res) == 1 else tuple(res)

    # ------------------------------------------------------------------ track progress (f110_track_*)
    TRACK_FIELDS = ("s", "ds", "lateral", "heading_error", "segment")

    def set_track(self, track, slot=0):
        """attach a raceline (a Track, an [M][2] array or a csv path) to map slot `slot`; returns the Track"""
        from .track import Track
        t = Track.coerce(track)
        xy = np.ascontiguousarray(t.xy, dtype=np.float64)
        check(_ffi.lib().f110_track_set(self._h, int(slot), dptr(xy), xy.shape[0], 1 if t.closed else 0), self._h)
        self.tracks = dict(getattr(self, "tracks", {}))
        self.tracks[int(slot)] = t
        if t.attrs is not None:    # (f110_track_set itself cleared the slot's attributes)
            self.set_track_attrs(slot, t.attrs)
        return t

    def set_track_attrs(self, slot, attrs):
        """per-point attributes of the track on `slot` for the preview's attr channels: [M][C] float64, M the track's point
        count, C in 1 .. 4; None clears them.  set_track uploads a Track's own attrs."""
        if attrs is None:
            check(_ffi.lib().f110_track_set_attrs(self._h, int(slot), None, 0, 0), self._h)
            return
        a = as_f64(attrs)
        if a.ndim != 2:
            raise ValueError("attrs must be [M][C]")
        check(_ffi.lib().f110_track_set_attrs(self._h, int(slot), dptr(a), a.shape[0], a.shape[1]), self._h)

    def enable_track(self, on=True):
        """with on, every step also produces the track columns (s, ds, lateral, heading_error, segment)"""
        check(_ffi.lib().f110_track_enable(self._h, 1 if on else 0), self._h)
        self.track_on = bool(on)

    def track_views(self):
        """the track columns in device memory: DeviceArrays [N] (float64; segment int32), stable for the handle's life"""
        v = _ffi.TrackViews()
        check(_ffi.lib().f110_track_views(self._h, C.byref(v)), self._h)
        N = self.N
        return {"s": DeviceArray(self, (N,), np.float64, v.s), "ds": DeviceArray(self, (N,), np.float64, v.ds),
                "lateral": DeviceArray(self, (N,), np.float64, v.lateral),
                "heading_error": DeviceArray(self, (N,), np.float64, v.heading_error),
                "segment": DeviceArray(self, (N,), np.int32, v.segment)}

    def get_track(self):
        """host copy of the last step's track columns"""
        N = self.N
        out = {k: np.empty(N) for k in self.TRACK_FIELDS[:4]}
        out["segment"] = np.empty(N, dtype=np.int32)
        o = _ffi.TrackHost(dptr(out["s"]), dptr(out["ds"]), dptr(out["lateral"]), dptr(out["heading_error"]), i32ptr(out["segment"]))
        check(_ffi.lib().f110_track_get(self._h, C.byref(o)), self._h)
        return out

    def track_host_block(self, fields=TRACK_FIELDS):
        """page-locked views step_host fills with the track columns (with the host block's completion semantics);
        returns {name: NumPy view}, overwritten by every step_host"""
        fields = tuple(fields)
        N = self.N
        views = {}
        o = _ffi.TrackHost()
        for f in fields:
            if f not in self.TRACK_FIELDS:
                raise KeyError(f)
            v = self.pinned_empty((N,), np.int32 if f == "segment" else np.float64)
            v[...] = 0
            views[f] = v
            setattr(o, f, i32ptr(v) if f == "segment" else dptr(v))
        check(_ffi.lib().f110_track_host_block(self._h, C.byref(o)), self._h)
        self._track_pinned = views   # (the block must outlive its registration)
        return views

    def track_project_batch(self, poses, slot=0):
        """unit form: host poses [m][3] on the track of `slot` -> [m][5] = s, lateral, heading_error, segment, t"""
        p = as_f64(poses)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("poses must be [m][3]")
        out = np.empty((p.shape[0], 5))
        check(_ffi.lib().f110_track_project_batch(self._h, int(slot), dptr(p), p.shape[0], dptr(out)), self._h)
        return out

    # ------------------------------------------------------------------ what the per-agent device forms share
    def _f32_out(self, shape, out, name="out"):
        """a device form's float32 output: a new DeviceArray of `shape` for None, else the caller's, which must be one"""
        if out is None:
            return DeviceArray(self, shape, np.float32)
        if not isinstance(out, DeviceArray) or tuple(out.shape) != shape or out.dtype != np.float32:
            raise ValueError("%s must be a float32 DeviceArray of shape %s" % (name, shape))
        return out

    @staticmethod
    def _pinned_ptr(shape, pinned):
        """the address of a pinned_empty float32 array of `shape` that also receives the output (None: no copy)"""
        if pinned is None:
            return None
        if not isinstance(pinned, np.ndarray) or pinned.dtype != np.float32 or tuple(pinned.shape) != shape or not pinned.flags.c_contiguous:
            raise ValueError("pinned must be a C-contiguous float32 array of shape %s (pinned_empty)" % (shape,))
        return pinned.ctypes.data

    @staticmethod
    def _opt(a, ptr=dptr):
        """an optional array argument: ptr(a), None for None"""
        return None if a is None else ptr(a)

    def _armed_list(self, agents, seed, agent_base):
        """what arming a feature takes: the agents (int32, strictly ascending; None: every agent) and their streams' words uint64
        [m][4], agent n's from PCG64(SeedSequence(seed, spawn_key=(agent_base + n,)))"""
        from .reset_sampler import stream_words
        a = np.arange(self.N, dtype=np.int32) if agents is None else np.ascontiguousarray(np.asarray(agents).reshape(-1), dtype=np.int32)
        if int(agent_base) < 0:
            raise ValueError("agent_base must be >= 0, got %d" % int(agent_base))
        if a.size == 0 or a.min() < 0 or a.max() >= self.N or np.any(np.diff(a) <= 0):
            raise ValueError("agents must be a strictly ascending list of 1 .. %d indices within 0 .. %d" % (self.N, self.N - 1))
        lo = int(a[0])
        return a, np.ascontiguousarray(stream_words(seed, int(a[-1]) - lo + 1, int(agent_base) + lo)[a - lo], dtype=np.uint64)

    @staticmethod
    def _stream_rows(streams, m, copy=False):
        """the streams argument uint64 [m][4]; copy: an array of its own, which the call then writes"""
        words = np.array(streams, dtype=np.uint64, order="C") if copy else np.ascontiguousarray(streams, dtype=np.uint64)
        if words.shape != (m, 4):
            raise ValueError("streams must be uint64 [%d][4]" % m)
        return words

    @staticmethod
    def _fresh_rows(fresh, m):
        """the unit forms' fresh argument int32 [m] (None: no row is fresh)"""
        if fresh is None:
            return None
        fr = np.ascontiguousarray(fresh, dtype=np.int32)
        if fr.shape != (m,):
            raise ValueError("fresh must be [m]")
        return fr

    @staticmethod
    def _start_rows(start):
        """the unit forms' start rows float64 [m][10], and m"""
        st = as_f64(start)
        if st.ndim != 2 or st.shape[1] != 10:
            raise ValueError("start must be [m][10] = state[7], FIFO newest, FIFO older, FIFO count")
        return st, st.shape[0]

    def _rollout_host(self, spec, actions, device_form):
        """a rollout on host candidates: uploaded, device_form(Rollout, d_actions) called, its DeviceArrays downloaded (a tuple)
        and freed"""
        from .rollout import Rollout
        ro = Rollout.coerce(spec)
        a = as_f64(actions)
        if tuple(a.shape) != ro.actions_shape(self.N):
            raise ValueError("actions must have shape %s" % (ro.actions_shape(self.N),))
        with DeviceArray(self, a.shape, np.float64) as d_act:
            d_act.upload(a)
            res = device_form(ro, d_act)
            res = res if isinstance(res, tuple) else (res,)
            host = tuple(r.download() for r in res)
            for r in res:
                r.free()
        return host

    # ------------------------------------------------------------------ track preview (f110_track_preview_*)
    def track_preview_device(self, preview, out=None, pinned=None):
        """the raceline ahead of every agent (track_preview.TrackPreview) as a float32 DeviceArray [N][P][D], from the s column
        and the pose of the step just taken.  `out`: a float32 DeviceArray of preview.shape(N) to reuse (None: a new one).
        Enqueued on the handle's stream, per env block behind a two-block step (no host wait).  pinned: a pinned_empty float32
        array of the same shape that also receives the result, complete after sync().  Needs enable_track()."""
        from .track_preview import TrackPreview
        pv = TrackPreview.coerce(preview)
        shape = pv.shape(self.N)
        out = self._f32_out(shape, out)
        pp = self._pinned_ptr(shape, pinned)
        spec = pv.spec()
        check(_ffi.lib().f110_track_preview_device(self._h, C.byref(spec), out.ptr, pp), self._h)
        return out

    def track_preview(self, poses, s, preview, slot=0, raw=False, segments=False):
        """unit form on host arrays: poses [m][3] and their arc lengths s [m] (track_project_batch's first column) on the track
        of `slot` -> float32 [m][P][D]; with raw also float64 [m][P][8] (every channel before scaling, absent attributes 0.0),
        with segments also int32 [m][P] (each station's segment)"""
        from .track_preview import TrackPreview
        pv = TrackPreview.coerce(preview)
        p = as_f64(poses)
        sv = np.asarray(s, dtype=np.float64).reshape(-1)
        if p.ndim != 2 or p.shape[1] != 3 or sv.shape[0] != p.shape[0]:
            raise ValueError("poses must be [m][3] and s [m]")
        m = p.shape[0]
        rows = np.ascontiguousarray(np.concatenate([p, sv[:, None]], axis=1))
        out = np.zeros(pv.shape(m), dtype=np.float32)
        rw = np.zeros((m, pv.points, 8)) if raw else None
        sg = np.zeros((m, pv.points), dtype=np.int32) if segments else None
        spec = pv.spec()
        check(_ffi.lib().f110_track_preview_batch(self._h, C.byref(spec), int(slot), dptr(rows), m, out.ctypes.data,
                                                  self._opt(rw), self._opt(sg, i32ptr)), self._h)
        return _with_extras(out, rw, sg)

    # ------------------------------------------------------------------ neighbours (f110_neighbors_*)
    def neighbors_device(self, spec, out=None, pinned=None):
        """every agent's K nearest opponents of its own env (neighbors.Neighbors) as a float32 DeviceArray [N][K][D], from the pose,
        the speed and (for 'gap_s') the s column of the step just taken.  `out`: a float32 DeviceArray of spec.shape(N) to reuse
        (None: a new one).  Enqueued on the handle's stream, per env block behind a two-block step (no host wait).  pinned: a
        pinned_empty float32 array of the same shape that also receives the result, complete after sync().  'gap_s' needs
        enable_track()."""
        from .neighbors import Neighbors
        nb = Neighbors.coerce(spec)
        shape = nb.shape(self.N)
        out = self._f32_out(shape, out)
        pp = self._pinned_ptr(shape, pinned)
        sp = nb.spec()
        check(_ffi.lib().f110_neighbors_device(self._h, C.byref(sp), out.ptr, pp), self._h)
        return out

    def neighbors(self, rows, spec, A, track_L=0.0, raw=False, indices=False):
        """unit form on host arrays: rows [m][5] = x, y, theta, v, s in env-major order, m a multiple of A (1 .. 256, whatever this
        handle's num_agents is); track_L > 0 wraps 'gap_s' as a closed track of that length -> float32 [m][K][D]; with raw also
        float64 [m][K][10] (every channel before scaling; an empty slot pad, 'valid' 0.0), with indices also int32 [m][K] (-1: empty)"""
        from .neighbors import Neighbors
        nb = Neighbors.coerce(spec)
        r = as_f64(rows)
        if r.ndim != 2 or r.shape[1] != 5:
            raise ValueError("rows must be [m][5] = x, y, theta, v, s")
        m = r.shape[0]
        out = np.zeros(nb.shape(m), dtype=np.float32)
        rw = np.zeros((m, nb.k, 10)) if raw else None
        ix = np.zeros((m, nb.k), dtype=np.int32) if indices else None
        sp = nb.spec()
        check(_ffi.lib().f110_neighbors_batch(self._h, C.byref(sp), int(A), float(track_L), dptr(r), m, out.ctypes.data,
                                              self._opt(rw), self._opt(ix, i32ptr)), self._h)
        return _with_extras(out, rw, ix)

    # ------------------------------------------------------------------ rollout (f110_rollout_*)
    def rollout_device(self, spec, d_actions, out=None, traj=None, pinned=None):
        """roll every agent's K candidates (rollout.Rollout) ahead from its live state: d_actions is a float64 DeviceArray of
        spec.actions_shape(N) = (steer, speed) per candidate and action.  Returns the summary, a float32 DeviceArray [N][K][D], or
        with spec.traj the pair (summary, trajectory [N][K][H][4]).  `out` / `traj`: DeviceArrays of those shapes to reuse (None: new
        ones).  Enqueued on the handle's stream, per env block behind a two-block step (no host wait).  pinned: a pinned_empty
        float32 array of the summary's shape that also receives it, complete after sync().  'progress' and 'end_lat' need a track
        on every map slot in use (set_track); tracking need not be enabled."""
        return self._rollout_device(spec, d_actions, out, traj, pinned)

    def _rollout_device(self, spec, d_actions, out, traj, pinned, opponents=None, opp=None):
        from .rollout import Rollout
        ro = Rollout.coerce(spec)
        shape, tshape, ashape = ro.shape(self.N), ro.traj_shape(self.N), ro.actions_shape(self.N)
        if not isinstance(d_actions, DeviceArray) or tuple(d_actions.shape) != ashape or d_actions.dtype != np.float64:
            raise ValueError("d_actions must be a float64 DeviceArray of shape %s" % (ashape,))
        out = self._f32_out(shape, out)
        if not ro.traj:
            if traj is not None:
                raise ValueError("traj is given, but the rollout does not ask for the trajectory")
        else:
            traj = self._f32_out(tshape, traj, "traj")
        pp = self._pinned_ptr(shape, pinned)
        sp = ro.spec()
        if opponents is None:
            check(_ffi.lib().f110_rollout_device(self._h, C.byref(sp), d_actions.ptr, out.ptr, traj.ptr if ro.traj else None, pp), self._h)
            return (out, traj) if ro.traj else out
        opp = self._f32_out((self.N, ro.k, 2), opp, "opp")
        osp = opponents.spec()
        check(_ffi.lib().f110_rollout_opp_device(self._h, C.byref(sp), C.byref(osp), d_actions.ptr, out.ptr, traj.ptr if ro.traj else None,
                                                 opp.ptr, pp), self._h)
        return (out, traj, opp) if ro.traj else (out, opp)

    def rollout_opp_device(self, spec, opponents, d_actions, out=None, traj=None, opp=None, pinned=None):
        """rollout_device with every candidate measured against the predicted motion of the other cars of its env
        (opponents.Opponents): returns (summary, opp) or with spec.traj (summary, trajectory, opp); opp is a float32
        DeviceArray [N][K][2] = (the smallest distance to a prediction, the first action within the radius of one, H when none).
        The summary and the trajectory are rollout_device's, bit for bit.  'track' mode needs a track on every map slot in use."""
        from .opponents import Opponents
        return self._rollout_device(spec, d_actions, out, traj, pinned, Opponents.coerce(opponents), opp)

    def rollout_opp(self, spec, opponents, actions):
        """rollout_opp_device on host candidates, returned as NumPy: (summary, opp float32 [N][K][2]), or with spec.traj (summary,
        trajectory, opp)"""
        return self._rollout_host(spec, actions, lambda ro, d_act: self.rollout_opp_device(ro, opponents, d_act))

    @staticmethod
    def _opp_rows(opp_rows, m):
        """the unit forms' opponent rows [m][Ao][4] = x, y, v, theta (None: no opponents)"""
        if opp_rows is None:
            return np.zeros((m, 0, 4)), 0
        r = as_f64(opp_rows)
        if r.ndim != 3 or r.shape[0] != m or r.shape[2] != 4:
            raise ValueError("opp_rows must be [m][Ao][4] = x, y, v, theta")
        return r, int(r.shape[1])

    def rollout_opp_rows(self, spec, opponents, start, actions, opp_rows, slot=0, params=None):
        """rollout_rows with the opponent term on host rows: opp_rows [m][Ao][4] = (x, y, v, theta) of each row's opponents (None:
        none) -> a dict: out, raw, traj, traj_raw as rollout_rows(raw=True) returns them (the trajectory entries None without
        spec.traj), pred float64 [m][Ao][H][2] the predictions (NaN: ignored), opp_raw float64 [m][K][2] = (OPP_MIN, OPP_FREE) and
        opp float32 [m][K][2] what the device form writes"""
        from .opponents import Opponents
        return self._rollout_rows(spec, start, actions, slot, params, True, Opponents.coerce(opponents), opp_rows)

    def rollout(self, spec, actions):
        """rollout_device on host candidates `actions` (spec.actions_shape(N)), returned as NumPy: the summary float32 [N][K][D],
        or with spec.traj the pair (summary, trajectory)"""
        host = self._rollout_host(spec, actions, self.rollout_device)
        return host if len(host) > 1 else host[0]

    def rollout_rows(self, spec, start, actions, slot=0, params=None, raw=False):
        """unit form on host rows: start [m][10] = state[7], the steering FIFO's newest and older entry and its fill count (0, 1, 2),
        all on map slot `slot`; params [m][18] (None: this handle's row of agent slot 0); actions spec.actions_shape(m) -> the summary
        float32 [m][K][D]; with spec.traj also the trajectory float32 [m][K][H][4]; with raw also float64 [m][K][10] (every channel
        before scaling; 'progress' and 'end_lat' 0.0 when the slot has no track) and, with spec.traj, the float64 trajectory"""
        return self._rollout_rows(spec, start, actions, slot, params, raw)

    def _rollout_rows(self, spec, start, actions, slot, params, raw, opponents=None, opp_rows=None):
        from .rollout import Rollout
        ro = Rollout.coerce(spec)
        st, m = self._start_rows(start)
        a = as_f64(actions)
        if tuple(a.shape) != ro.actions_shape(m):
            raise ValueError("actions must have shape %s" % (ro.actions_shape(m),))
        pv = None
        if params is not None:
            pv = as_f64(params)
            if tuple(pv.shape) != (m, 18):
                raise ValueError("params must be [m][18]")
        out = np.zeros(ro.shape(m), dtype=np.float32)
        rw = np.zeros((m, ro.k, 10)) if raw else None
        tr = np.zeros(ro.traj_shape(m), dtype=np.float32) if ro.traj else None
        trw = np.zeros(ro.traj_shape(m)) if ro.traj and raw else None
        sp, opt = ro.spec(), self._opt
        trp = None if tr is None else tr.ctypes.data
        if opponents is None:
            check(_ffi.lib().f110_rollout_batch(self._h, C.byref(sp), int(slot), dptr(st), opt(pv), dptr(a), m, out.ctypes.data, opt(rw), trp,
                                                opt(trw)), self._h)
            return _with_extras(out, tr, rw, trw)
        orows, Ao = self._opp_rows(opp_rows, m)
        pred, oraw, o32 = np.zeros((m, Ao, ro.horizon, 2)), np.zeros((m, ro.k, 2)), np.zeros((m, ro.k, 2), dtype=np.float32)
        osp = opponents.spec()
        check(_ffi.lib().f110_rollout_opp_batch(self._h, C.byref(sp), C.byref(osp), int(slot), dptr(st), opt(pv), dptr(a), dptr(orows) if Ao else None, Ao, m,
                                                out.ctypes.data, dptr(rw), trp, opt(trw), dptr(pred) if Ao else None, dptr(oraw),
                                                o32.ctypes.data), self._h)
        return dict(out=out, raw=rw, traj=tr, traj_raw=trw, pred=pred, opp_raw=oraw, opp=o32)

    # ------------------------------------------------------------------ MPPI planner (f110_mppi_*)
    mppi_planner, mppi_agents = None, None

    def set_mppi(self, spec, agents=None, seed=0, agent_base=0):
        """arm the planner (mppi.Mppi or a dict of its settings) on `agents` (indices into the N agents, strictly ascending; None:
        every agent).  Agent n draws from PCG64(SeedSequence(seed, spawn_key=(agent_base + n,))): agent_base is the handle's first
        agent in a larger run (a shard), so that the run draws the same numbers however it is split.  Every nominal starts as
        (0, v_init); nothing is launched.  The planner acts in mppi_device and in step_host(scripted=True).  Returns the Mppi."""
        from .mppi import Mppi
        mp = Mppi.coerce(spec)
        a, words = self._armed_list(agents, seed, agent_base)
        sp = mp.spec()
        check(_ffi.lib().f110_mppi_set(self._h, C.byref(sp), i32ptr(a), int(a.size), u64ptr(words)), self._h)
        self.mppi_planner, self.mppi_agents, self.mppi_opponents = mp, a, None
        return mp

    def clear_mppi(self):
        """disarm the planner and free its memory (the opponent term attached to it goes with it)"""
        check(_ffi.lib().f110_mppi_set(self._h, None, None, 0, None), self._h)
        self.mppi_planner, self.mppi_agents, self.mppi_opponents = None, None, None

    mppi_opponents = None

    def set_mppi_opponents(self, opp, w_hit=0.0, w_near=0.0, near_ref=0.0):
        """attach the opponent term (opponents.Opponents or a dict of its settings) to the armed planner: every
        candidate then also costs w_hit * (actions from its first sample within the radius of a predicted opponent to the horizon)
        + w_near * max(near_ref - its smallest distance to a prediction, 0).  Nothing is launched; mppi_device and
        step_host(scripted=True) use it from the next call on.  set_mppi and clear_mppi drop it.  Returns the Opponents."""
        from .opponents import Opponents, check_weights
        op = Opponents.coerce(opp)
        w_hit, w_near, near_ref = check_weights(w_hit, w_near, near_ref)
        sp = op.spec()
        check(_ffi.lib().f110_mppi_set_opponents(self._h, C.byref(sp), w_hit, w_near, near_ref), self._h)
        self.mppi_opponents = (op, w_hit, w_near, near_ref)
        return op

    def clear_mppi_opponents(self):
        """detach the opponent term; the planner stays armed"""
        check(_ffi.lib().f110_mppi_set_opponents(self._h, None, 0.0, 0.0, 0.0), self._h)
        self.mppi_opponents = None

    def mppi_device(self, d_actions, info=None):
        """one planning call: the armed agents' rows of the device action buffer [N][2] (float64, the step's layout) are written
        from their live state; the other rows are left alone.  info: a float32 DeviceArray [N][4] whose armed rows receive
        mppi.INFO = (the lowest cost, the nominal's cost, the effective sample size, the index of the lowest cost).  Enqueued on
        the handle's stream, per env block behind a two-block step (no host wait)."""
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        ip = None if info is None else self._f32_out((self.N, 4), info, "info").ptr
        check(_ffi.lib().f110_mppi_device(self._h, a, ip), self._h)

    def mppi(self, actions, info=False):
        """mppi_device on a host action array [N][2]: a copy with the armed agents' rows replaced (and, with info, float32 [N][4],
        zero in the other rows)"""
        act = as_f64(actions, (self.N, 2))
        with DeviceArray(self, (self.N, 2), np.float64) as d_act, DeviceArray(self, (self.N, 4), np.float32) as d_info:
            d_act.upload(act)
            d_info.upload(np.zeros((self.N, 4), dtype=np.float32))
            self.mppi_device(d_act, d_info)
            out, inf = d_act.download(), d_info.download()
        return (out, inf) if info else out

    def get_mppi_state(self):
        """(nominal float64 [M][H][2], streams uint64 [M][4]) of the armed planner, in the armed list's order: what to keep next to
        a state blob"""
        mp = self.mppi_planner
        if mp is None:
            raise _ffi.F110LibraryError("no planner is armed (set_mppi)")
        nom = np.zeros(mp.nominal_shape(self.mppi_agents.size))
        words = np.zeros((self.mppi_agents.size, 4), dtype=np.uint64)
        check(_ffi.lib().f110_mppi_get(self._h, dptr(nom), u64ptr(words)), self._h)
        return nom, words

    def set_mppi_state(self, nominal=None, streams=None):
        """restore get_mppi_state's arrays, or seed the nominal (from a policy's prior, say): values must be finite and within
        the planner's bounds.  None leaves that part alone."""
        mp = self.mppi_planner
        if mp is None:
            raise _ffi.F110LibraryError("no planner is armed (set_mppi)")
        m = self.mppi_agents.size
        nom = None if nominal is None else as_f64(nominal, mp.nominal_shape(m))
        words = None if streams is None else self._stream_rows(streams, m)
        check(_ffi.lib().f110_mppi_put(self._h, self._opt(nom), self._opt(words, u64ptr)), self._h)

    def mppi_rows(self, spec, start, nominal, streams, slot=0, params=None, fresh=None):
        """unit form on host rows (the same kernels; the armed planner is not touched): start [m][10] as rollout_rows takes it,
        nominal [m][H][2], streams uint64 [m][4], params [m][18] (None: this handle's row of agent slot 0), fresh int32 [m] (the
        rows' step_count: 0 = a fresh row; None: none is).  Returns a dict: actions [m][2], info float32 [m][4], candidates
        [m][K][H][2], cost [m][K], weight [m][K], nominal and streams after the call."""
        return self._mppi_rows(spec, start, nominal, streams, slot, params, fresh)

    def mppi_opp_rows(self, spec, opponents, w_hit, w_near, near_ref, start, nominal, streams, opp_rows, slot=0, params=None, fresh=None):
        """mppi_rows with the opponent term on host rows: opp_rows [m][Ao][4] = (x, y, v, theta) of each row's opponents (None:
        none).  The dict also holds opp_raw float64 [m][K][2] = the candidates' (OPP_MIN, OPP_FREE)."""
        from .opponents import Opponents, check_weights
        return self._mppi_rows(spec, start, nominal, streams, slot, params, fresh, Opponents.coerce(opponents),
                               check_weights(w_hit, w_near, near_ref), opp_rows)

    def _mppi_rows(self, spec, start, nominal, streams, slot, params, fresh, opponents=None, weights=None, opp_rows=None):
        from .mppi import Mppi
        mp = Mppi.coerce(spec)
        st, m = self._start_rows(start)
        nom = as_f64(nominal, mp.nominal_shape(m)).copy()
        words = self._stream_rows(streams, m, copy=True)
        pv = None if params is None else as_f64(params, (m, 18))
        fr = self._fresh_rows(fresh, m)
        act, inf = np.zeros((m, 2)), np.zeros((m, 4), dtype=np.float32)
        cand, cost, wgt = np.zeros((m, mp.k, mp.horizon, 2)), np.zeros((m, mp.k)), np.zeros((m, mp.k))
        sp, opt = mp.spec(), self._opt
        res = dict(actions=act, info=inf, candidates=cand, cost=cost, weight=wgt, nominal=nom, streams=words)
        if opponents is None:
            check(_ffi.lib().f110_mppi_batch(self._h, C.byref(sp), int(slot), dptr(st), opt(pv), opt(fr, i32ptr), m, dptr(nom), u64ptr(words), dptr(act),
                                             inf.ctypes.data, dptr(cand), dptr(cost), dptr(wgt)), self._h)
            return res
        orows, Ao = self._opp_rows(opp_rows, m)
        oraw = np.zeros((m, mp.k, 2))
        osp = opponents.spec()
        check(_ffi.lib().f110_mppi_opp_batch(self._h, C.byref(sp), C.byref(osp), weights[0], weights[1], weights[2], int(slot), dptr(st), opt(pv),
                                             opt(fr, i32ptr), dptr(orows) if Ao else None, Ao, m, dptr(nom), u64ptr(words), dptr(act), inf.ctypes.data,
                                             dptr(cand), dptr(cost), dptr(wgt), dptr(oraw)), self._h)
        res["opp_raw"] = oraw
        return res

    # ------------------------------------------------------------------ particle filter (f110_pf_*)
    pf_filter, pf_agents = None, None

    def set_particle_filter(self, spec, agents=None, seed=0, agent_base=0):
        """arm the filter (particle_filter.ParticleFilter or a dict of its settings) on `agents` (indices into the N agents, strictly
        ascending; None: every agent).  Agent n draws from PCG64(SeedSequence(seed, spawn_key=(agent_base + n,))): agent_base is the
        handle's first agent in a larger run (a shard), so that the run draws the same numbers however it is split.  Every cloud
        starts as zeros with uniform weights and becomes a cloud around its car at the first call after a reset (or through
        set_pf_state); nothing is launched.  The filter acts in localize_device.  Returns the ParticleFilter."""
        from .particle_filter import ParticleFilter
        pf = ParticleFilter.coerce(spec)
        pf.check_beams(self.B)
        a, words = self._armed_list(agents, seed, agent_base)
        sp = pf.spec()
        check(_ffi.lib().f110_pf_set(self._h, C.byref(sp), i32ptr(a), int(a.size), u64ptr(words)), self._h)
        self.pf_filter, self.pf_agents = pf, a
        return pf

    def clear_particle_filter(self):
        """disarm the filter and free its memory"""
        check(_ffi.lib().f110_pf_set(self._h, None, None, 0, None), self._h)
        self.pf_filter, self.pf_agents = None, None

    def localize_device(self, d_pose, d_info=None):
        """one localisation call: the armed agents' rows of the float64 DeviceArray d_pose [N][3] receive the estimate (x, y, theta)
        from their live scan and the pose's move since the last call; the other rows are left alone.  d_info: a float32 DeviceArray
        [N][4] whose armed rows receive particle_filter.INFO = (the effective sample size, the cloud's spread in metres, the
        estimate's distance from the true pose, 1 if the cloud was resampled).  Enqueued on the handle's stream, per env block
        behind a two-block step (no host wait)."""
        if isinstance(d_pose, DeviceArray):
            if tuple(d_pose.shape) != (self.N, 3) or d_pose.dtype != np.float64:
                raise ValueError("d_pose must be a float64 DeviceArray of shape %s" % ((self.N, 3),))
            p = d_pose.ptr
        else:
            p = int(d_pose)
        ip = None if d_info is None else self._f32_out((self.N, 4), d_info, "d_info").ptr
        check(_ffi.lib().f110_pf_device(self._h, p, ip), self._h)

    def localize(self):
        """localize_device into fresh host arrays: (pose float64 [N][3], info float32 [N][4]), NaN in the rows that are not armed"""
        with DeviceArray(self, (self.N, 3), np.float64) as d_pose, DeviceArray(self, (self.N, 4), np.float32) as d_info:
            d_pose.upload(np.full((self.N, 3), np.nan))
            d_info.upload(np.full((self.N, 4), np.nan, dtype=np.float32))
            self.localize_device(d_pose, d_info)
            return d_pose.download(), d_info.download()

    def _pf_armed(self):
        if self.pf_filter is None:
            raise _ffi.F110LibraryError("no filter is armed (set_particle_filter)")
        return self.pf_filter, self.pf_agents.size

    def get_pf_state(self):
        """(particles float64 [M][P][3], weights [M][P], last [M][3], streams uint64 [M][4]) of the armed filter, in the armed
        list's order: what to keep next to a state blob"""
        pf, m = self._pf_armed()
        X, W, last = np.zeros(pf.cloud_shape(m)), np.zeros((m, pf.particles)), np.zeros((m, 3))
        words = np.zeros((m, 4), dtype=np.uint64)
        check(_ffi.lib().f110_pf_get(self._h, dptr(X), dptr(W), dptr(last), u64ptr(words)), self._h)
        return X, W, last, words

    def set_pf_state(self, particles=None, weights=None, last=None, streams=None):
        """restore get_pf_state's arrays, or seed the clouds: particles must be finite, a weight row finite, >= 0 and with a sum
        above 0.  None leaves that part alone."""
        pf, m = self._pf_armed()
        X = None if particles is None else as_f64(particles, pf.cloud_shape(m))
        W = None if weights is None else as_f64(weights, (m, pf.particles))
        la = None if last is None else as_f64(last, (m, 3))
        words = None if streams is None else self._stream_rows(streams, m)
        opt = self._opt
        check(_ffi.lib().f110_pf_put(self._h, opt(X), opt(W), opt(la), opt(words, u64ptr)), self._h)

    def localize_rows(self, spec, poses, scans, particles, weights, last, streams, slot=0, fresh=None):
        """unit form on host rows (the same kernels; the armed filter is not touched): poses [m][3] the true poses on map slot
        `slot`, scans [m][num_beams], particles [m][P][3], weights [m][P], last [m][3], streams uint64 [m][4], fresh int32 [m] (the
        rows' step_count: 0 = a fresh row; None: none is).  Returns a dict: pose [m][3], info float32 [m][4], noise [m][P][3],
        ancestors int32 [m][P], expected [m][P][B'], logw [m][P], and particles, weights, last and streams after the call."""
        from .particle_filter import ParticleFilter
        pf = ParticleFilter.coerce(spec)
        pf.check_beams(self.B)
        po = as_f64(poses)
        if po.ndim != 2 or po.shape[1] != 3:
            raise ValueError("poses must be [m][3]")
        m, P = po.shape[0], pf.particles
        sc = as_f64(scans, (m, self.B))
        X, W, la = as_f64(particles, pf.cloud_shape(m)).copy(), as_f64(weights, (m, P)).copy(), as_f64(last, (m, 3)).copy()
        words = self._stream_rows(streams, m, copy=True)
        fr = self._fresh_rows(fresh, m)
        pose, inf = np.zeros((m, 3)), np.zeros((m, 4), dtype=np.float32)
        noise, anc = np.zeros((m, P, 3)), np.zeros((m, P), dtype=np.int32)
        expect, logw = np.zeros((m, P, pf.n_beams)), np.zeros((m, P))
        sp = pf.spec()
        check(_ffi.lib().f110_pf_batch(self._h, C.byref(sp), int(slot), dptr(po), dptr(sc), self._opt(fr, i32ptr), m, dptr(X), dptr(W),
                                       dptr(la), u64ptr(words), dptr(pose), inf.ctypes.data, dptr(noise), i32ptr(anc),
                                       dptr(expect), dptr(logw)), self._h)
        return dict(pose=pose, info=inf, noise=noise, ancestors=anc, expected=expect, logw=logw, particles=X, weights=W, last=la, streams=words)

    # ------------------------------------------------------------------ rendering (f110_render_device)
    def render_device(self, agents=None, width=64, height=64, view='ego', m_per_px=0.05, center=(0.0, 0.0), angle=0.0,
                      fwd_offset=0.0, layers=('map', 'cars'), car_size=None, rgb=False, palette=None, out=None):
        """class images of the last observation, one frame per camera agent (None: every agent): uint8 DeviceArrays
        classes [F][H][W] (render.CLASSES) and, with rgb, [F][H][W][3] = palette[classes] -> classes or (classes, rgb).
        view 'world' (center, angle), 'follow' (the agent's pose + fwd_offset along its heading, north up) or 'ego' (heading
        up); layers from ('map', 'track', 'scan', 'cars') or 'all'; car_size (length, width) overrides every agent's params.
        Enqueued on the handle's stream (no host wait); `out` = (classes[, rgb]) DeviceArrays to reuse."""
        from . import render as R
        spec = R.make_spec(width, height, view, m_per_px, center, angle, fwd_offset, layers, car_size)
        a = R.check_agents(agents, self.N, spec)
        pal = R.check_palette(palette)
        F, H, W = a.size, spec.height, spec.width
        if out is not None:
            out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            want = [((F, H, W), np.uint8)] + ([((F, H, W, 3), np.uint8)] if rgb else [])
            if len(out) != len(want) or any(tuple(o.shape) != s or o.dtype != d for o, (s, d) in zip(out, want)):
                raise ValueError("out must be %s DeviceArrays of shapes %s" % (len(want), [s for s, _ in want]))
            cls, img = out[0], (out[1] if rgb else None)
        else:
            cls = DeviceArray(self, (F, H, W), np.uint8)
            img = DeviceArray(self, (F, H, W, 3), np.uint8) if rgb else None
        ap = None if agents is None else a.ctypes.data_as(_ffi._i32p)
        check(_ffi.lib().f110_render_device(self._h, C.byref(spec), ap, F, cls.ptr, img.ptr if img is not None else None,
                                            pal.ctypes.data_as(_ffi._u8p)), self._h)
        return (cls, img) if rgb else cls

    def render(self, agents=None, **spec):
        """render_device, downloaded (synchronises): NumPy uint8 classes [F][H][W], or (classes, rgb) with rgb=True"""
        res = self.render_device(agents, **spec)
        res = res if isinstance(res, tuple) else (res,)
        try:
            host = tuple(r.download() for r in res)
        finally:
            for r in res:
                r.free()
        return host if len(host) > 1 else host[0]

    # ------------------------------------------------------------------ compact observations (f110_obs_encode_*)
    def encode_obs_device(self, enc, out=None, fill=False, pinned=None):
        """the last step's observation as float32 [N][F][D] (obs_encoder.ObsEncoder), newest frame last: the frames of `out`
        move down by one and the new frame goes last; agents that start an episode (step_count 1), or all with fill, get
        every frame set to it.  `out` is the caller's stack (a float32 DeviceArray of enc.shape(N)); None: one buffer per
        encoder, allocated (and filled) on the first call and reused from then on.  Enqueued on the handle's stream, per env
        block behind a two-block step (no host wait).  pinned: a pinned_empty float32 array of the same shape that also
        receives the stack, complete after sync()."""
        from .obs_encoder import ObsEncoder
        enc = ObsEncoder.coerce(enc)
        enc.check_beams(self.B)
        shape = enc.shape(self.N)
        if out is None:
            out = self._obs_stacks.get(id(enc))
            if out is None or out[0] is not enc or out[1].ptr is None:
                out = (enc, DeviceArray(self, shape, np.float32))   # (the encoder is held: its id stays its own)
                self._obs_stacks[id(enc)] = out
                fill = True
            out = out[1]
        else:
            out = self._f32_out(shape, out)
        pp = self._pinned_ptr(shape, pinned)
        spec = enc.spec(fill)
        check(_ffi.lib().f110_obs_encode_device(self._h, C.byref(spec), out.ptr, pp), self._h)
        return out

    def encode_obs(self, enc, out=None, fill=False):
        """encode_obs_device, downloaded (synchronises): NumPy float32 [N][F][D]"""
        return self.encode_obs_device(enc, out, fill).download()

    def obs_encode_batch(self, enc, scans, cols, step_count, stack, fill=False):
        """unit form on host arrays: scans [m][B], cols [m][8] (the eight feature sources in obs_encoder.FEATURES order),
        step_count [m], stack float32 [m][F][D] -> the updated stack (a new array)"""
        from .obs_encoder import ObsEncoder
        enc = ObsEncoder.coerce(enc)
        enc.check_beams(self.B)
        scans, cols = as_f64(scans), as_f64(cols)
        m = scans.shape[0]
        if scans.shape != (m, self.B) or cols.shape != (m, 8):
            raise ValueError("scans must be [m][%d] and cols [m][8]" % self.B)
        sc = np.ascontiguousarray(step_count, dtype=np.int32)
        st = np.array(stack, dtype=np.float32, order="C")
        if sc.shape != (m,) or st.shape != enc.shape(m):
            raise ValueError("step_count must be [m] and stack %s" % (enc.shape(m),))
        spec = enc.spec(fill)
        check(_ffi.lib().f110_obs_encode_batch(self._h, C.byref(spec), dptr(scans), dptr(cols), i32ptr(sc), m, st.ctypes.data), self._h)
        return st

    # ------------------------------------------------------------------ scripted cars (f110_controllers_set / f110_follow_gap_*)
    def set_controllers(self, assign, controllers):
        """arm follow-the-gap controllers: `controllers` a list of 1 .. 8 gap_follower.GapFollower (or dicts of their settings),
        `assign` int32 [N] (or [E][A]): -1 = external, else the index of the agent's controller.  Nothing is launched; the
        controllers act in follow_gap_device and in step_host(scripted=True)."""
        from .gap_follower import GapFollower, MAX_SPECS
        ctrls = [GapFollower.coerce(c) for c in controllers]
        if not (1 <= len(ctrls) <= MAX_SPECS):
            raise ValueError("1 .. %d controllers, got %d" % (MAX_SPECS, len(ctrls)))
        a = np.ascontiguousarray(np.asarray(assign).reshape(-1), dtype=np.int32)
        if a.shape != (self.N,):
            raise ValueError("assign must hold one entry per agent (%d), got %d" % (self.N, a.size))
        specs = (_ffi.GapFollowerSpec * len(ctrls))(*[c.spec(self.B) for c in ctrls])
        check(_ffi.lib().f110_controllers_set(self._h, specs, len(ctrls), i32ptr(a)), self._h)
        self.controllers, self.controller_assign = ctrls, a

    def clear_controllers(self):
        """disarm the controllers"""
        check(_ffi.lib().f110_controllers_set(self._h, None, 0, None), self._h)
        self.controllers, self.controller_assign = [], None

    def follow_gap_device(self, d_actions):
        """the armed controllers write their agents' rows of the device action buffer [N][2] from the last step's scans; the
        other rows are left alone.  Enqueued on the handle's stream, per env block behind a two-block step (no host wait)."""
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_follow_gap_device(self._h, a), self._h)

    def follow_gap(self, scans, controller=None, step_count=None, info=False):
        """unit form on host arrays: scans [m][B] -> actions [m][2] (and, with info, int32 [m][5]: closest beam, bubble
        half-width, gap start, gap end, target beam, relative to the window; -1s for a blocked row).  step_count [m]: rows
        with 0 get (0, 0)."""
        from .gap_follower import GapFollower
        c = GapFollower() if controller is None else GapFollower.coerce(controller)
        scans = as_f64(scans)
        m = scans.shape[0]
        if scans.shape != (m, self.B):
            raise ValueError("scans must be [m][%d]" % self.B)
        sc = None
        if step_count is not None:
            sc = np.ascontiguousarray(step_count, dtype=np.int32)
            if sc.shape != (m,):
                raise ValueError("step_count must be [m]")
        act = np.zeros((m, 2))
        inf = np.zeros((m, 5), dtype=np.int32) if info else None
        spec = c.spec(self.B)
        check(_ffi.lib().f110_follow_gap_batch(self._h, C.byref(spec), dptr(scans), None if sc is None else i32ptr(sc), m, dptr(act),
                                               None if inf is None else i32ptr(inf)), self._h)
        return (act, inf) if info else act

    # ------------------------------------------------------------------ scripted cars on the line (f110_line_followers_set / f110_follow_line_*)
    def set_line_followers(self, assign, followers):
        """arm line followers: `followers` a list of 1 .. 8 line_follower.LineFollower (or dicts of their settings), `assign`
        int32 [N] (or [E][A]): -1 = no line follower, else the index of the agent's follower.  Nothing is launched; they act in
        follow_line_device and in step_host(scripted=True), on the track of the agent's map slot (tracking must be on then)."""
        from .line_follower import LineFollower, MAX_SPECS
        fs = [LineFollower.coerce(c) for c in followers]
        if not (1 <= len(fs) <= MAX_SPECS):
            raise ValueError("1 .. %d line followers, got %d" % (MAX_SPECS, len(fs)))
        a = np.ascontiguousarray(np.asarray(assign).reshape(-1), dtype=np.int32)
        if a.shape != (self.N,):
            raise ValueError("assign must hold one entry per agent (%d), got %d" % (self.N, a.size))
        specs = (_ffi.LineFollowerSpec * len(fs))(*[c.spec() for c in fs])
        check(_ffi.lib().f110_line_followers_set(self._h, specs, len(fs), i32ptr(a)), self._h)
        self.line_followers, self.line_follower_assign = fs, a

    def clear_line_followers(self):
        """disarm the line followers"""
        check(_ffi.lib().f110_line_followers_set(self._h, None, 0, None), self._h)
        self.line_followers, self.line_follower_assign = [], None

    def follow_line_device(self, d_actions, info=None):
        """the armed line followers write their agents' rows of the device action buffer [N][2] from the last step's track
        columns; the other rows are left alone.  info: a float64 DeviceArray [N][4] (ld, vref, k, lim) whose armed rows are
        written too.  Enqueued on the handle's stream, per env block behind a two-block step (no host wait)."""
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        ip = None
        if info is not None:
            if not isinstance(info, DeviceArray) or tuple(info.shape) != (self.N, 4) or info.dtype != np.float64:
                raise ValueError("info must be a float64 DeviceArray of shape %s" % ((self.N, 4),))
            ip = info.ptr
        check(_ffi.lib().f110_follow_line_device(self._h, a, ip), self._h)

    def follow_line(self, rows, follower=None, A=1, slot=0, raw=False):
        """unit form on host rows, on the track of map slot `slot`: rows [m][7] = x, y, theta, v, s, lateral, step_count,
        env-major with A cars per env -> actions [m][2] (and, with raw, float64 [m][12]: line_follower.RAW).  It does not
        project: s and lateral come from track_project."""
        from .line_follower import LineFollower
        c = LineFollower() if follower is None else LineFollower.coerce(follower)
        rows = as_f64(rows)
        if rows.ndim != 2 or rows.shape[1] != 7 or rows.shape[0] % int(A) != 0:
            raise ValueError("rows must be [m][7] with m a multiple of A = %d" % int(A))
        m = rows.shape[0]
        act = np.zeros((m, 2))
        rw = np.zeros((m, _ffi.LINE_NRAW)) if raw else None
        spec = c.spec()
        check(_ffi.lib().f110_follow_line_batch(self._h, C.byref(spec), int(slot), int(A), dptr(rows), m, dptr(act), self._opt(rw)), self._h)
        return (act, rw) if raw else act

    # ------------------------------------------------------------------ the reference's example policy
    def pure_pursuit_batch(self, waypoints, poses, lookahead, vgain, wheelbase, max_reacquire=20.0):
        """PurePursuitPlanner.plan (examples/waypoint_follow.py:203-217) for host poses [m][3];
        waypoints [M][3] = (x, y, speed).  Returns actions [m][2] = (steer, speed)."""
        wp = as_f64(waypoints); poses = as_f64(poses)
        if wp.ndim != 2 or wp.shape[1] != 3 or poses.ndim != 2 or poses.shape[1] != 3:
            raise ValueError("waypoints must be [M][3] = (x, y, speed) and poses [m][3]")
        out = np.empty((poses.shape[0], 2))
        check(_ffi.lib().f110_pure_pursuit_batch(self._h, dptr(wp), wp.shape[0], dptr(poses), poses.shape[0], float(lookahead),
                                                 float(vgain), float(wheelbase), float(max_reacquire), dptr(out)), self._h)
        return out

    def pure_pursuit_device(self, d_waypoints, num_waypoints, d_actions, lookahead, vgain, wheelbase, max_reacquire=20.0):
        """the same policy on the live poses of all N agents, device buffers, no host round trip"""
        w = d_waypoints.ptr if isinstance(d_waypoints, DeviceArray) else int(d_waypoints)
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_pure_pursuit_device(self._h, w, int(num_waypoints), float(lookahead), float(vgain), float(wheelbase),
                                                  float(max_reacquire), a), self._h)

    def pure_pursuit_poses_device(self, d_waypoints, num_waypoints, d_poses, d_actions, lookahead, vgain, wheelbase, max_reacquire=20.0):
        """the same policy on poses held in device memory, d_poses float64 [N][3] (localize_device's estimates, say) instead of the
        live poses; a NaN pose gets (0, 4.0)"""
        w = d_waypoints.ptr if isinstance(d_waypoints, DeviceArray) else int(d_waypoints)
        p = d_poses.ptr if isinstance(d_poses, DeviceArray) else int(d_poses)
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_pure_pursuit_poses_device(self._h, w, int(num_waypoints), p, float(lookahead), float(vgain), float(wheelbase),
                                                        float(max_reacquire), a), self._h)

    def scan_policy_device(self, d_actions, steer_gain=0.5, steer_max=0.4189, sector_limit=1.75, v_lo=1.0, v_hi=6.0, d_ref=6.0):
        """a reactive policy that reads the step's scans where they are (f110_scan_policy_device: steer towards the most open
        sector, speed from the clearance ahead) and writes the device action buffer — no host round trip"""
        a = d_actions.ptr if isinstance(d_actions, DeviceArray) else int(d_actions)
        check(_ffi.lib().f110_scan_policy_device(self._h, float(steer_gain), float(steer_max), float(sector_limit), float(v_lo), float(v_hi),
                                                 float(d_ref), a), self._h)

    def scan_path_stats(self, enable=None, read=True):
        """diagnostics: rays marched as dict(fast, guard, exact) since the last read; enable=True/False
        switches the counting (off by default)"""
        out = np.zeros(3, dtype=np.int64)
        check(_ffi.lib().f110_scan_path_stats(self._h, -1 if enable is None else int(bool(enable)),
                                              out.ctypes.data_as(_ffi._i64p) if read else None), self._h)
        return dict(fast=int(out[0]), guard=int(out[1]), exact=int(out[2]))

    def beam_dir_index_batch(self, thetas):
        thetas = as_f64(thetas).reshape(-1)
        idx = np.empty((thetas.shape[0], self.B), dtype=np.int32)
        check(_ffi.lib().f110_beam_dir_index_batch(self._h, dptr(thetas), thetas.shape[0], i32ptr(idx)), self._h)
        return idx

    def dynamics_batch(self, x, u, params):
        x = as_f64(x); u = as_f64(u); pv = _ffi.params_vector(params) if isinstance(params, dict) else as_f64(params, (18,))
        m = x.shape[0]
        x = as_f64(x, (m, 7)); u = as_f64(u, (m, 2))
        f_st = np.empty((m, 7)); f_ks = np.empty((m, 5))
        check(_ffi.lib().f110_dynamics_batch(self._h, dptr(x), dptr(u), dptr(pv), m, dptr(f_st), dptr(f_ks)), self._h)
        return f_st, f_ks

    def pid_batch(self, inputs, params):
        inputs = as_f64(inputs); pv = _ffi.params_vector(params) if isinstance(params, dict) else as_f64(params, (18,))
        m = inputs.shape[0]
        inputs = as_f64(inputs, (m, 4))
        out = np.empty((m, 2))
        check(_ffi.lib().f110_pid_batch(self._h, dptr(inputs), dptr(pv), m, dptr(out)), self._h)
        return out

    def update_pose_batch(self, state0, buf0, cnt0, actions, params, time_step, integrator, lidar_dist):
        state0 = as_f64(state0); m = state0.shape[0]
        state0 = as_f64(state0, (m, 7)); buf0 = as_f64(buf0, (m, 2)); actions = as_f64(actions, (m, 2))
        cnt0 = np.ascontiguousarray(cnt0, dtype=np.int32)
        pv = _ffi.params_vector(params) if isinstance(params, dict) else as_f64(params, (18,))
        s1 = np.empty((m, 7)); b1 = np.empty((m, 2)); c1 = np.empty((m,), dtype=np.int32); sp = np.empty((m, 3))
        check(_ffi.lib().f110_update_pose_batch(self._h, dptr(state0), dptr(buf0), i32ptr(cnt0), dptr(actions),
                                                dptr(pv), float(time_step), int(integrator), float(lidar_dist),
                                                m, dptr(s1), dptr(b1), i32ptr(c1), dptr(sp)), self._h, SyntaxError)
        return s1, b1, c1, sp

    def get_vertices_batch(self, poses, length, width):
        poses = as_f64(poses); m = poses.shape[0]
        poses = as_f64(poses, (m, 3))
        out = np.empty((m, 4, 2))
        check(_ffi.lib().f110_get_vertices_batch(self._h, dptr(poses), float(length), float(width), m, dptr(out)), self._h)
        return out

    def gjk_batch(self, va, vb):
        va = as_f64(va); m = va.shape[0]
        va = as_f64(va, (m, 4, 2)); vb = as_f64(vb, (m, 4, 2))
        flags = np.empty((m,), dtype=np.int32)
        check(_ffi.lib().f110_gjk_batch(self._h, dptr(va), dptr(vb), m, i32ptr(flags)), self._h)
        return flags

    def collision_multiple_batch(self, vertices):
        vertices = as_f64(vertices)
        g, n = vertices.shape[0], vertices.shape[1]
        vertices = as_f64(vertices, (g, n, 4, 2))
        col = np.empty((g, n)); idx = np.empty((g, n))
        check(_ffi.lib().f110_collision_multiple_batch(self._h, dptr(vertices), g, n, dptr(col), dptr(idx)), self._h)
        return col, idx

    def ttc_batch(self, scans, vels, ttc_thresh=0.005):
        scans = as_f64(scans); m = scans.shape[0]
        scans = as_f64(scans, (m, self.B)); vels = as_f64(vels, (m,))
        flags = np.empty((m,), dtype=np.int32)
        check(_ffi.lib().f110_ttc_batch(self._h, dptr(scans), dptr(vels), m, float(ttc_thresh), i32ptr(flags)), self._h)
        return flags

    def raycast_batch(self, ego, vertices, scans):
        ego = as_f64(ego); m = ego.shape[0]
        ego = as_f64(ego, (m, 3)); vertices = as_f64(vertices, (m, 4, 2))
        out = np.array(scans, dtype=np.float64, order='C')
        if out.shape != (m, self.B):
            raise ValueError("scans must be [M][num_beams]")
        mm = np.empty((m, 2), dtype=np.int32)
        check(_ffi.lib().f110_raycast_batch(self._h, dptr(ego), dptr(vertices), m, dptr(out), i32ptr(mm)), self._h)
        return out, mm

    def get_range_batch(self, rows):
        rows = as_f64(rows); m = rows.shape[0]
        rows = as_f64(rows, (m, 8))
        out = np.empty((m,))
        check(_ffi.lib().f110_get_range_batch(self._h, dptr(rows), m, dptr(out)), self._h)
        return out

    _HELPER_WIDTHS = {   # op -> (in width as a function of n, out width)
        _ffi.OP_ACCL_CONSTRAINTS: (lambda n: 6, 1), _ffi.OP_STEERING_CONSTRAINT: (lambda n: 6, 1), _ffi.OP_CROSS: (lambda n: 4, 1),
        _ffi.OP_ARE_COLLINEAR: (lambda n: 6, 1), _ffi.OP_PERPENDICULAR: (lambda n: 2, 2), _ffi.OP_TRIPLE_PRODUCT: (lambda n: 6, 2),
        _ffi.OP_AVG_POINT: (lambda n: 2 * n, 2), _ffi.OP_FURTHEST_POINT: (lambda n: 2 * n + 2, 1), _ffi.OP_SUPPORT: (lambda n: 4 * n + 2, 2),
        _ffi.OP_GET_TRMTX: (lambda n: 3, 16), _ffi.OP_XY_2_RC: (lambda n: 9, 2), _ffi.OP_DISTANCE_TRANSFORM: (lambda n: 2, 1),
        _ffi.OP_TRACE_RAY: (lambda n: 3, 1)}

    def helper_batch(self, op, rows, n=4):
        """f110_helper_batch: `rows` [M][in width of op] -> [M][out width] (the small star-exported functions, include/f110.h)"""
        in_w, out_w = self._HELPER_WIDTHS[op]
        rows = as_f64(rows)
        m = rows.shape[0]
        rows = as_f64(rows, (m, in_w(int(n))))
        out = np.empty((m, out_w))
        check(_ffi.lib().f110_helper_batch(self._h, int(op), dptr(rows), m, int(n), dptr(out)), self._h)
        return out

    def dt_from_bitmap(self, bitmap, resolution):
        """get_dt (laser_models.py:40-53): resolution * exact EDT of `bitmap` (nonzero = free), on the device"""
        img = np.ascontiguousarray(np.asarray(bitmap) != 0, dtype=np.uint8)
        if img.ndim != 2:
            raise ValueError("bitmap must be 2-D")
        out = np.empty(img.shape)
        check(_ffi.lib().f110_dt_from_bitmap(self._h, img.ctypes.data_as(_ffi._u8p), img.shape[0], img.shape[1], float(resolution), dptr(out)), self._h)
        return out

    def edt_sq(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        out = np.empty(img.shape, dtype=np.uint32)
        check(_ffi.lib().f110_edt_sq(self._h, img.ctypes.data_as(_ffi._u8p), img.shape[0], img.shape[1],
                                     out.ctypes.data_as(_ffi._u32p)), self._h)
        return out
