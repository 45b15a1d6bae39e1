"""The observation encoder's rule (include/f110.h, f110_obs_spec) in NumPy float64, cast with astype(np.float32).

This is the model every device result is held to bit for bit (tests/test_obs_encoder_host.py, tests/test_gpu_obs_encoder.py).
It is written from the rule, not from the kernel: vectorised over agents, a Python loop over sectors, and for MEAN an
explicit ascending loop over the beams of a sector (np.sum adds pairwise, which is a different rounding).
"""
import numpy as np

FEATURES = ("vx", "steer", "yaw_rate", "slip", "collision", "lateral", "heading_error", "ds")


def sector_bounds(W, K, beam_lo=0):
    """[(b0, b1)] of the K sectors of beams [beam_lo, beam_lo + W): integer arithmetic"""
    return [(beam_lo + (k * W) // K, beam_lo + ((k + 1) * W) // K) for k in range(K)]


def new_frame(scans, cols, sectors, pool, beams, features, range_clip, range_scale, scales):
    """scans [m][B] float64, cols [m][8] float64 (FEATURES order) -> float32 [m][D]"""
    scans = np.asarray(scans, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.float64)
    m, B = scans.shape
    lo, hi = (0, B) if beams is None else beams
    out = []
    with np.errstate(all="ignore"):
        for b0, b1 in sector_bounds(hi - lo, sectors, lo) if sectors else []:
            if pool == "min":
                v = np.min(scans[:, b0:b1], axis=1)
            elif pool == "mean":
                v = scans[:, b0].copy()
                for b in range(b0 + 1, b1):
                    v = v + scans[:, b]
                v = v / np.float64(b1 - b0)
            elif pool == "center":
                v = scans[:, (b0 + b1 - 1) >> 1]
            else:
                raise ValueError(pool)
            out.append((np.minimum(v, np.float64(range_clip)) / np.float64(range_scale)).astype(np.float32))
        for c, name in enumerate(FEATURES):
            if name in features:
                out.append((cols[:, c] / np.float64(scales.get(name, 1.0))).astype(np.float32))
    return np.stack(out, axis=1) if out else np.empty((m, 0), dtype=np.float32)


def update_stack(stack, frame, step_count, fill):
    """the frame rule: stack float32 [m][F][D], frame [m][D], step_count [m] -> the new stack.  An agent with step_count 1
    (or every agent with fill) gets all F frames set to the new frame; every other agent's frames move down by one."""
    stack = np.asarray(stack, dtype=np.float32)
    out = np.concatenate([stack[:, 1:], frame[:, None, :]], axis=1)
    start = np.ones(stack.shape[0], dtype=bool) if fill else (np.asarray(step_count) == 1)
    out[start] = frame[start][:, None, :]
    return out


def encode(enc, scans, cols, step_count, stack, fill=False):
    """one encode call of an f1tenth_gym_amd.ObsEncoder `enc` (only its settings are read)"""
    frame = new_frame(scans, cols, enc.sectors, enc.pool, enc.beams, enc.features, enc.range_clip, enc.range_scale, enc.scales)
    return update_stack(stack, frame, step_count, fill)


def bits(a):
    """the uint32 view the comparisons are made on (NaN patterns included)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the unit grid both test files walk (host harness and GPU unit form) ----
GRID_K = (1, 7, 64, 108, 270, 1080)
GRID_B = (1080, 4096, 61)
GRID_FRAMES = ((1, False), (4, False), (4, True), (1, True))   # (F, fill)
ALL_FEATURES = FEATURES


def unit_grid():
    """(B, beams, K, pool, F, fill) over K x B (non-divisible widths) x {all beams, a sub-range} x the three pools x F / fill;
    K is kept where it does not exceed the beams used (the rule refuses the rest)"""
    for B in GRID_B:
        for beams in (None, (B // 7, B - B // 5)):
            W = B if beams is None else beams[1] - beams[0]
            for K in GRID_K:
                if K > W:
                    continue
                for pool in ("min", "mean", "center"):
                    for F, fill in GRID_FRAMES:
                        yield B, beams, K, pool, F, fill


def random_inputs(rng, m, B, F, D, clip=30.0):
    """rows with ranges below and above the clip, +inf and NaN sprinkled in (never -inf: inf - inf makes a NaN whose sign differs
    between x86 and the GPU, and a lidar range is never negative), feature sources of both signs, step_count cycling through
    0, 1, 2, and a stack of arbitrary finite float32 content (so a shift that moves the wrong floats shows)"""
    scans = rng.uniform(0.05, 1.2 * clip, size=(m, B))
    scans[rng.random((m, B)) < 0.01] = np.inf
    scans[rng.random((m, B)) < 0.01] = np.nan
    scans[0] = rng.uniform(0.05, 0.9 * clip, size=B)      # one row entirely finite and below the clip
    cols = rng.normal(0.0, 3.0, size=(m, 8))
    cols[:, 4] = rng.integers(0, 2, size=m)                # the collisions column holds 0. / 1.
    step_count = (np.arange(m) % 3).astype(np.int32)
    stack = rng.normal(0.0, 1.0, size=(m, F, D)).astype(np.float32)
    return scans, cols, step_count, stack
