"""NumPy restatement of the raceline rule (include/f110.h, f110_raceline_batch): the authority the device kernel, the
host program (tests/host_harness/raceline_main.hip) and BatchSim.raceline are compared with, bit for bit.

Independent of f1tenth_gym_amd/raceline.py; it shares only centerline.resample_closed.  float64 throughout, every operation in the
order the header states (NumPy does not fuse), whole-array operations for what is order-free and plain loops for the two running
sums.
"""
import math

import numpy as np

from f1tenth_gym_amd.centerline import resample_closed

MAX_POINTS = 4096
DEFAULTS = dict(spacing=0.4, levels=4, iters=200, margin=0.3, v_max=8.0, a_lat=7.0, a_accel=7.0, a_brake=8.0)


def spec(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def momentum(iters):
    """beta[k] = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2"""
    beta = np.empty(int(iters))
    t = 1.0
    for k in range(int(iters)):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * (t * t))) / 2.0
        beta[k] = (t - 1.0) / t1
        t = t1
    return beta


def station_count(L, spacing, levels):
    return (1 << levels) * max(8, int(math.floor(L / (spacing * (1 << levels)) + 0.5)))


def stations(track, spacing=0.4, levels=4):
    """the uniform stations of a closed Track with a 'half_width' column: (q [M][2], w [M])"""
    col = track.attrs[:, track.attr_names.index('half_width')]
    M = station_count(track.length, spacing, levels)
    q, w, _, _ = resample_closed(track.xy, col, track.length / M)
    assert q.shape[0] == M
    return q, w


def _running(v):
    cum = np.empty(v.shape[0])
    acc = 0.0
    for k in range(v.shape[0]):
        cum[k] = acc
        acc += float(v[k])
    return cum, acc


def frame(q, w, margin):
    """step 1: (normals [M][2], bounds [M], the lengths l [M])"""
    d = np.roll(q, -1, axis=0) - np.roll(q, 1, axis=0)
    l = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    with np.errstate(all='ignore'):
        n = np.stack([-d[:, 1] / l, d[:, 0] / l], axis=1)
    return n, np.maximum(w - margin, 0.0), l


def clamp(x, lo, hi):
    return np.minimum(np.maximum(x, lo), hi)


def offsets(q, n, b, levels, iters, beta):
    """step 2"""
    M = q.shape[0]
    alpha = np.zeros(M)
    for lv in range(levels, -1, -1):
        s = 1 << lv
        idx = np.arange(0, M, s)
        if lv < levels:
            odd = np.arange(s, M, 2 * s)
            alpha[odd] = clamp(0.5 * (alpha[odd - s] + alpha[(odd + s) % M]), -b[odd], b[odd])
        qa, na, ba = q[idx], n[idx], b[idx]
        al = alpha[idx].copy()
        y = al.copy()
        for k in range(iters):
            p = qa + y[:, None] * na
            r = (np.roll(p, 1, axis=0) - 2.0 * p) + np.roll(p, -1, axis=0)
            g = (np.roll(r, 1, axis=0) - 2.0 * r) + np.roll(r, -1, axis=0)
            gg = 2.0 * (na[:, 0] * g[:, 0] + na[:, 1] * g[:, 1])
            new = clamp(y - (1.0 / 32.0) * gg, -ba, ba)
            y = new + beta[k] * (new - al)
            al = new
        alpha[idx] = al
    return alpha


def curvature(p):
    """centerline.curvature_closed's formula in its operation order (restated: the rule is part of the contract)"""
    a, c = np.roll(p, 1, axis=0), np.roll(p, -1, axis=0)
    ab, bc, ac = p - a, c - p, c - a
    cross = ab[:, 0] * bc[:, 1] - ab[:, 1] * bc[:, 0]
    den = np.sqrt(ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]) * np.sqrt(bc[:, 0] * bc[:, 0] + bc[:, 1] * bc[:, 1]) * np.sqrt(ac[:, 0] * ac[:, 0] + ac[:, 1] * ac[:, 1])
    with np.errstate(all='ignore'):
        return 2.0 * cross / den


def ceiling(kappa, v_max, a_lat):
    with np.errstate(divide='ignore'):
        return np.minimum(v_max * v_max, a_lat / np.abs(kappa))


def profile(c, cum, L, a_accel, a_brake):
    """step 4 -> vx"""
    inf = np.array([np.inf])
    ka = 2.0 * a_accel
    A = ka * cum
    F = c - A
    pre = np.minimum.accumulate(F)
    suf = np.concatenate([np.minimum.accumulate(F[::-1])[::-1][1:], inf])
    up = np.minimum(A + pre, (A + ka * L) + suf)
    kb = 2.0 * a_brake
    B = kb * cum
    G = c + B
    sufg = np.minimum.accumulate(G[::-1])[::-1]
    preg = np.concatenate([inf, np.minimum.accumulate(G)[:-1]])
    um = np.minimum(sufg - B, (preg + kb * L) - B)
    return np.sqrt(np.minimum(c, np.minimum(up, um)))


def lap_time(ln, vx):
    t = (2.0 * ln) / (vx + np.roll(vx, -1))
    acc = 0.0
    for v in t:
        acc += float(v)
    return acc


def check(q, w, levels, iters, margin, v_max, a_lat, a_accel, a_brake):
    """the refusals before the solve: None, or the reason"""
    M = q.shape[0]
    if not (np.all(np.isfinite(q)) and np.all(np.isfinite(w))):
        return "non-finite input"
    if not (0 <= levels <= 6):
        return "levels"
    if not (0 <= iters <= 4096):
        return "iters"
    if M > MAX_POINTS:
        return "M > 4096"
    if M % (1 << levels):
        return "M not a multiple of 2^levels"
    if M // (1 << levels) < 8:
        return "M / 2^levels < 8"
    for v in (v_max, a_lat, a_accel, a_brake):
        if not (math.isfinite(v) and v > 0):
            return "limits"
    if not (math.isfinite(margin) and margin >= 0):
        return "margin"
    return None


def raceline(q, w, levels=4, iters=200, margin=0.3, v_max=8.0, a_lat=7.0, a_accel=7.0, a_brake=8.0, spacing=None):
    """the rule for one line -> dict(alpha, xy, kappa, vx, length, lap_time, b, n, seg_len, cum), or ValueError on a refusal"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    why = check(q, w, levels, iters, margin, v_max, a_lat, a_accel, a_brake)
    if why:
        raise ValueError(why)
    n, b, l = frame(q, w, margin)
    if not np.all(l > 0.0):
        raise ValueError("zero-length q[i+1] - q[i-1]")
    alpha = offsets(q, n, b, levels, iters, momentum(iters))
    p = q + alpha[:, None] * n
    d = np.roll(p, -1, axis=0) - p
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    if not np.all(ln > 0.0):
        raise ValueError("zero-length raceline segment")
    kappa = curvature(p)
    if not np.all(np.isfinite(kappa)):
        raise ValueError("a curvature of the raceline is not finite")
    cum, L = _running(ln)
    c = ceiling(kappa, v_max, a_lat)
    vx = profile(c, cum, L, a_accel, a_brake)
    return dict(alpha=alpha, xy=p, kappa=kappa, vx=vx, length=L, lap_time=lap_time(ln, vx), b=b, n=n, seg_len=ln, cum=cum, c=c)


def sweep(c, ln, a_accel, a_brake, laps=2):
    """the forward / backward pass in v^2, sequentially, `laps` times round: what profile()'s closed form is checked against"""
    M = c.shape[0]
    v2 = c.copy()
    for _ in range(laps):
        for i in range(M):
            j = (i + 1) % M
            v2[j] = min(v2[j], v2[i] + 2.0 * a_accel * ln[i])
    for _ in range(laps):
        for j in range(M - 1, -1, -1):
            k = (j + 1) % M
            v2[j] = min(v2[j], v2[k] + 2.0 * a_brake * ln[j])
    return np.sqrt(v2)


def ellipse(M, a=12.0, b=7.0, width=1.0, phase=0.5):
    """a synthetic closed line of M points: an ellipse with a few harmonics on its radius, counter-clockwise, and half widths that
    vary along it -> (q [M][2], w [M]).  At M = 8 the points are ~8 m apart; the rule does not care."""
    phi = 2.0 * np.pi * np.arange(M, dtype=np.float64) / M
    r = 1.0 + 0.15 * np.cos(2.0 * phi + phase) + 0.08 * np.cos(3.0 * phi + 2.0 * phase) + 0.04 * np.sin(5.0 * phi)
    q = np.stack([a * r * np.cos(phi), b * r * np.sin(phi)], axis=1)
    return np.ascontiguousarray(q), width * (1.0 + 0.3 * np.cos(phi + 1.0))


def stadium(n_straight, n_arc, length=20.0, radius=5.0, width=1.0):
    """a stadium: two straights along x whose points share their y exactly (curvature exactly 0 inside them) and two half circles;
    2 * (n_straight + n_arc) points -> (q, w)"""
    xs = -0.5 * length + length * np.arange(n_straight, dtype=np.float64) / n_straight
    th = np.pi * np.arange(n_arc, dtype=np.float64) / n_arc
    bottom = np.stack([xs, np.full(n_straight, -radius)], axis=1)
    right = np.stack([0.5 * length + radius * np.sin(th), -radius * np.cos(th)], axis=1)
    top = np.stack([-xs, np.full(n_straight, radius)], axis=1)
    left = np.stack([-0.5 * length - radius * np.sin(th), radius * np.cos(th)], axis=1)
    q = np.ascontiguousarray(np.concatenate([bottom, right, top, left]))
    return q, np.full(q.shape[0], float(width))


def objective(q, n, alpha):
    p = q + alpha[:, None] * n
    r = (np.roll(p, 1, axis=0) - 2.0 * p) + np.roll(p, -1, axis=0)
    return float(np.sum(r * r))
