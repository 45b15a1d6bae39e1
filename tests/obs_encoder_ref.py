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


# ---- the launch forms the host chooses (f110_hip.hip, obs_plan_lds) --------------------------------------------------------------
LDS_BYTES = 65536     # what one workgroup may ask for as dynamic LDS


def _align16(n):
    return (n + 15) & ~15


def planned_lds(W, F, D):
    """bytes of LDS one wave needs with the row staged: the W doubles of the window and the stack image of F * D + 3 floats (the
    three spare floats let the image sit at the agent's phase), each rounded up to 16 bytes"""
    return _align16(8 * W) + _align16(4 * (F * D + 3))


def planned_staged(W, F, D):
    """the staging rule restated: the row goes through LDS while it fits next to the stack image in 64 KiB; otherwise
    k_obs_encode<false> walks the sectors in HBM.  (Without sectors there is no row: that is not on this grid.)"""
    return planned_lds(W, F, D) <= LDS_BYTES


FIVE_FEATURES = FEATURES[:5]


def launch_form_grid():
    """(B, beams, K, pool, F, fill, features, staged): the boundaries of the staging rule and the frame counts the unit grid
    does not reach.  `staged` is written down by hand; tests/test_obs_encoder_host.py holds planned_staged to it for every row.

    With all 4096 beams the row takes 32768 bytes, so the image may take 32768: F * D + 3 <= 8192.  F * D = 8189 would be the
    last staged product, but 8189 = 19 * 431 has no factor F <= 16 with D <= 4096 + 8, so no encoder has it.  Rounding to 16
    bytes makes F * D = 8186 .. 8189 all ask for exactly 65536 bytes: F * D = 8188 (F = 4, D = 2047 and F = 2, D = 4094) is the
    largest product an encoder can have on the staged side, and F * D = 8190 (F = 2, D = 4095) the smallest on the other."""
    rows = [
        # the smallest unstaged case: one sector over 8192 beams, one frame, no feature
        (8192, None, 1, "min", 1, False, (), False),
        # W = 8190 with F * D = 1 asks for 65520 + 16 = 65536 bytes, the last staged window; W = 8191 is the first unstaged one
        (8192, (1, 8191), 1, "mean", 1, False, (), True),
        (8192, (2, 8192), 1, "center", 1, True, (), True),
        (8192, (1, 8192), 1, "mean", 1, False, (), False),
        (8192, (0, 8191), 1, "center", 1, True, (), False),
        # 4096 beams: F * D = 8188 staged with exactly 65536 bytes, F * D = 8190 unstaged (see above for 8189)
        (4096, None, 2039, "min", 4, False, FEATURES, True),
        (4096, None, 4094, "mean", 2, False, (), True),
        (4096, None, 4090, "min", 2, False, FIVE_FEATURES, False),
        (4096, None, 4095, "mean", 2, True, (), False),
        # F * D = 8192, the cap itself: every beam its own sector, and 16 frames of 504 sectors + 8 features for the three pools
        (4096, None, 4096, "center", 2, False, (), False),
        (4096, None, 4096, "min", 2, False, (), False),
        (4096, None, 504, "min", 16, False, FEATURES, False),
        (4096, None, 504, "mean", 16, True, FEATURES, False),
        (4096, None, 504, "center", 16, False, FEATURES, False),
    ]
    # unstaged with a window that does not start at beam 0: the HBM walk must start at beam_lo.  4095 beams round up to the
    # same 32768 bytes as 4096; a window of 8192 of 8200 beams is unstaged whatever F * D is (2043 sectors of four or five beams: a
    # walk that starts seven beams early changes every one of them, whatever the pool)
    for pool in ("min", "mean", "center"):
        rows.append((4096, (1, 4096), 504, pool, 16, False, FEATURES, False))
        rows.append((8200, (7, 8199), 2043, pool, 4, pool == "mean", FIVE_FEATURES, False))
    # F in {5, 8, 16} at the everyday shape, staged, both fill values.  An agent's phase is (i F D) mod 4: with F = 5 and an odd
    # D the agents of a row take all four phases, with D = 110 phases 0 and 2; 8 D and 16 D are multiples of 4 whatever D is
    for F in (5, 8, 16):
        for fill in (False, True):
            rows.append((1080, None, 108, "min" if fill else "mean", F, fill, FIVE_FEATURES, True))
            rows.append((1080, (90, 990), 108, "center", F, fill, ("steer", "ds"), True))
    return rows


def launch_form_encoder(cls, row, scales):
    """the ObsEncoder (class handed in: this module needs no package import) of a launch_form_grid row"""
    B, beams, K, pool, F, fill, feats, _ = row
    return cls(sectors=K, pool=pool, beams=beams, features=feats, frames=F, range_clip=30.0, range_scale=7.0 if F % 2 else 30.0,
               scales=scales, num_beams=B)


def launch_form_inputs(rng, m, row, D):
    """random_inputs for a launch_form_grid row.  With a handful of sectors over thousands of beams nearly every sector of a
    row with 1 % NaN pools to NaN, which would compare NaN with NaN: the odd agents' rows are made finite (a fresh range where
    random_inputs put inf or NaN), the even ones keep them, and agent 0 stays below the clip as random_inputs leaves it"""
    scans, cols, step_count, stack = random_inputs(rng, m, row[0], row[4], D)
    fresh = rng.uniform(0.05, 36.0, size=scans.shape)
    odd = np.zeros(scans.shape, dtype=bool)
    odd[1::2] = True
    scans = np.where(odd & ~np.isfinite(scans), fresh, scans)
    return scans, cols, step_count, stack
