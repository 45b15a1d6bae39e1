"""NumPy restatement of the centreline rule of include/f110.h (f110_map_centerline): the passes with shifted boolean
arrays, the loop pick and the trace with plain loops, and the host post-processing of f1tenth_gym_amd/centerline.py with plain
loops.  TEST TOOLING: the reference the host program and the device are compared with, cell for cell.

Masks are bool [H][W] in table coordinates (row 0 at the bottom); an image (top row first, free where > 128) goes through
free_from_image first.
"""
import collections

import numpy as np

# P2 .. P9 as (dr, dc)
NBR = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


class Refused(Exception):
    """the refusals of the rule; .kind in 'seed', 'no_loop', 'not_simple', 'not_converged'"""

    def __init__(self, kind, msg, **info):
        Exception.__init__(self, msg)
        self.kind = kind
        self.info = info


def free_from_image(img):
    return np.flipud(np.asarray(img)) > 128


def shifted(m, dr, dc):
    """out[r][c] = m[r + dr][c + dc], False outside"""
    H, W = m.shape
    out = np.zeros_like(m)
    r0, r1 = max(0, -dr), min(H, H - dr)
    c0, c1 = max(0, -dc), min(W, W - dc)
    out[r0:r1, c0:c1] = m[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def neighbours(m):
    return [shifted(m, dr, dc) for dr, dc in NBR]


def counts(P):
    """(B, A) of every cell"""
    B = np.zeros(P[0].shape, dtype=np.int32)
    A = np.zeros(P[0].shape, dtype=np.int32)
    for i in range(8):
        B += P[i]
        A += ~P[i] & P[(i + 1) % 8]
    return B, A


def thin_subpass(m, sub):
    P2, P3, P4, P5, P6, P7, P8, P9 = P = neighbours(m)
    B, A = counts(P)
    if sub == 0:
        cond = ~(P2 & P4 & P6) & ~(P4 & P6 & P8)
    else:
        cond = ~(P2 & P4 & P8) & ~(P2 & P6 & P8)
    return m & (B >= 2) & (B <= 6) & (A == 1) & cond


def stair_pass(m, k):
    P2, P3, P4, P5, P6, P7, P8, P9 = neighbours(m)
    if k == 0:
        return m & P2 & P4 & ~(P6 | P7 | P8)
    if k == 1:
        return m & P4 & P6 & ~(P8 | P9 | P2)
    if k == 2:
        return m & P6 & P8 & ~(P2 | P3 | P4)
    return m & P8 & P2 & ~(P4 | P5 | P6)


def prune_pass(m):
    _, A = counts(neighbours(m))
    return m & (A <= 1)


def skeleton(free, max_passes=None):
    """steps 1 - 3 -> (final mask, deleted int64 [3], passes (thinning pairs, prune passes) with the empty one included)"""
    H, W = free.shape
    max_passes = 4 * (H + W) if max_passes is None or max_passes <= 0 else int(max_passes)
    m = free.copy()
    deleted = np.zeros(3, dtype=np.int64)
    passes = [0, 0]
    while True:
        if passes[0] == max_passes:
            raise Refused('not_converged', "thinning has not converged within max_passes = %d" % max_passes)
        n = 0
        for sub in (0, 1):
            d = thin_subpass(m, sub)
            n += int(d.sum())
            m = m & ~d
        passes[0] += 1
        deleted[0] += n
        if n == 0:
            break
    for k in range(4):
        d = stair_pass(m, k)
        deleted[1] += int(d.sum())
        m = m & ~d
    while True:
        if passes[1] == max_passes:
            raise Refused('not_converged', "pruning has not converged within max_passes = %d" % max_passes)
        d = prune_pass(m)
        n = int(d.sum())
        m = m & ~d
        passes[1] += 1
        deleted[2] += n
        if n == 0:
            break
    return m, deleted, tuple(passes)


def seed_cell(seed, H, W, res, origin):
    """step 4's transform; origin = (ox, oy, yaw).  None: outside the table"""
    ox, oy = float(origin[0]), float(origin[1])
    oc, os_ = float(np.cos(origin[2])), float(np.sin(origin[2]))
    xt, yt = float(seed[0]) - ox, float(seed[1]) - oy
    xr, yr = xt * oc + yt * os_, -xt * os_ + yt * oc
    if not (xr >= 0 and xr < W * res and yr >= 0 and yr < H * res):
        return None
    return min(int(yr / res), H - 1), min(int(xr / res), W - 1)


def component(free, cell):
    """the 8-connected free component of a cell, as a mask"""
    H, W = free.shape
    out = np.zeros_like(free)
    out[cell] = True
    q = collections.deque([cell])
    while q:
        r, c = q.popleft()
        for dr, dc in NBR:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and free[rr, cc] and not out[rr, cc]:
                out[rr, cc] = True
                q.append((rr, cc))
    return out


def pick_start(free, final, cell):
    H, W = free.shape
    if not free[cell]:
        raise Refused('seed', "the seed cell %r is not free" % (cell,))
    seen = np.zeros_like(free)
    seen[cell] = True
    q = collections.deque([cell])
    while q:
        r, c = q.popleft()
        if final[r, c]:
            return r, c
        for dr, dc in NBR:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and free[rr, cc] and not seen[rr, cc]:
                seen[rr, cc] = True
                q.append((rr, cc))
    raise Refused('no_loop', "no loop is reachable from the seed")


def set_neighbours(final, r, c):
    H, W = final.shape
    return [(i, (r + dr, c + dc)) for i, (dr, dc) in enumerate(NBR) if 0 <= r + dr < H and 0 <= c + dc < W and final[r + dr, c + dc]]


def trace(final, start, heading_table=None):
    """step 5: the ordered cells [n][2] from START; heading_table = (hx, hy) in the table frame or None (counter-clockwise)"""
    members, q, seen = [], collections.deque([start]), {start}
    branching, simple = 0, True
    while q:
        cell = q.popleft()
        members.append(cell)
        nb = set_neighbours(final, *cell)
        branching += len(nb) > 2
        simple = simple and len(nb) == 2
        for _, o in nb:
            if o not in seen:
                seen.add(o)
                q.append(o)
    if not simple:
        raise Refused('not_simple', "not a simple loop: %d of %d cells have more than two neighbours" % (branching, len(members)),
                      branching=branching, members=len(members))
    (i1, n1), (i2, n2) = set_neighbours(final, *start)
    first = n1
    if heading_table is not None:
        hx, hy = heading_table
        d1 = float(NBR[i1][1]) * hx + float(NBR[i1][0]) * hy
        d2 = float(NBR[i2][1]) * hx + float(NBR[i2][0]) * hy
        if d2 > d1:
            first = n2
    cells, prev, cur = [start], start, first
    while cur != start:
        cells.append(cur)
        nxt = [o for _, o in set_neighbours(final, *cur) if o != prev][0]
        prev, cur = cur, nxt
    assert len(cells) == len(members)
    if heading_table is None:
        area2 = 0
        for i in range(len(cells)):
            (r0, c0), (r1, c1) = cells[i], cells[(i + 1) % len(cells)]
            area2 += c0 * r1 - c1 * r0
        if area2 < 0:
            cells = cells[:1] + cells[1:][::-1]
    return np.array(cells, dtype=np.int32)


def centerline(free, T, res, origin, seed=(0.0, 0.0), heading=None, max_passes=None, whole=True):
    """the whole call: -> (cells int32 [n][2], half_width [n], deleted int64 [3], final mask).  whole=False thins the seed's free
    component only (the same loop; deleted and the mask then cover that component alone).  Refusals in the call's order."""
    H, W = free.shape
    if not (np.isfinite(seed[0]) and np.isfinite(seed[1])) or (heading is not None and not np.isfinite(heading)):
        raise Refused('seed', "the seed is not finite")
    cell = seed_cell(seed, H, W, res, origin)
    if cell is None:
        raise Refused('seed', "the seed lies outside the table")
    if not free[cell]:
        raise Refused('seed', "the seed cell %r is not free" % (cell,))
    if whole:
        final, deleted, _ = skeleton(free, max_passes)
    else:   # the component alone, thinned inside its bounding box (cells outside a mask count as not set: nothing changes)
        comp = component(free, cell)
        rows, cols = np.flatnonzero(comp.any(axis=1)), np.flatnonzero(comp.any(axis=0))
        r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
        part, deleted, _ = skeleton(comp[r0:r1, c0:c1], 4 * (H + W) if max_passes is None else max_passes)
        final = np.zeros_like(free)
        final[r0:r1, c0:c1] = part
    start = pick_start(free, final, cell)
    ht = None
    if heading is not None:
        oc, os_ = float(np.cos(origin[2])), float(np.sin(origin[2]))
        ct, st = float(np.cos(heading)), float(np.sin(heading))
        ht = (ct * oc + st * os_, -ct * os_ + st * oc)
    cells = trace(final, start, ht)
    return cells, np.asarray(T)[cells[:, 0], cells[:, 1]].astype(np.float64), deleted, final


def edt_table(free, res):
    """T of a mask by brute force over the occupied cells: res * sqrt(d2), exact for the small fixtures (the device's EDT is exact)"""
    H, W = free.shape
    occ = np.argwhere(~free)
    rr, cc = np.mgrid[0:H, 0:W]
    d2 = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    for k in range(0, occ.shape[0], 512):
        o = occ[k:k + 512]
        d = (rr[..., None] - o[:, 0]) ** 2 + (cc[..., None] - o[:, 1]) ** 2
        d2 = np.minimum(d2, d.min(axis=2))
    return res * np.sqrt(d2.astype(np.float64))


# ---- the host post-processing of f1tenth_gym_amd/centerline.py, restated with plain loops -------------------------------------
def post_process(cells, half_width, frame, spacing, smooth):
    """-> (points [M][2], half_width [M], kappa [M], stations [M], L)"""
    res, ox, oy, oc, os_ = frame
    n = len(cells)
    raw = np.empty((n, 2))
    for i, (r, c) in enumerate(cells):
        px, py = (float(c) + 0.5) * res, (float(r) + 0.5) * res
        raw[i] = (ox + (px * oc - py * os_), oy + (px * os_ + py * oc))

    def lengths(p):
        out = np.empty(len(p))
        for i in range(len(p)):
            d = p[(i + 1) % len(p)] - p[i]
            out[i] = np.sqrt(d[0] * d[0] + d[1] * d[1])
        return out

    L0 = 0.0
    for v in lengths(raw):
        L0 += float(v)
    m = min(int(np.floor(0.5 * float(smooth) * n / L0 + 0.5)), (n - 1) // 2)
    sm = raw.copy()
    if m > 0:
        for i in range(n):
            acc = np.zeros(2)
            for o in range(-m, m + 1):
                acc = acc + raw[(i + o) % n]
            sm[i] = acc / float(2 * m + 1)
    ln = lengths(sm)
    cum, L = np.empty(n), 0.0
    for i in range(n):
        cum[i] = L
        L += float(ln[i])
    M = max(3, int(np.floor(L / float(spacing) + 0.5)))
    pts, hw, st = np.empty((M, 2)), np.empty(M), np.empty(M)
    for j in range(M):
        s = float(j) * (L / M)
        k = 0
        while k + 1 < n and cum[k + 1] <= s:
            k += 1
        t = (s - cum[k]) / ln[k]
        k1 = (k + 1) % n
        pts[j] = sm[k] + t * (sm[k1] - sm[k])
        hw[j] = half_width[k] + t * (half_width[k1] - half_width[k])
        st[j] = s
    kappa = np.empty(M)
    for j in range(M):
        a, b, c = pts[(j - 1) % M], pts[j], pts[(j + 1) % M]
        ab, bc, ac = b - a, c - b, c - a
        cross = ab[0] * bc[1] - ab[1] * bc[0]
        den = np.sqrt(ab[0] * ab[0] + ab[1] * ab[1]) * np.sqrt(bc[0] * bc[0] + bc[1] * bc[1]) * np.sqrt(ac[0] * ac[0] + ac[1] * ac[1])
        kappa[j] = 2.0 * cross / den
    return pts, hw, kappa, st, L


# ---- fixtures: 96 x 130 uint8 images (top row first; 255 free, 0 occupied).  The width is no multiple of 64 and every corridor
# crosses columns 63 / 64.
H0, W0 = 96, 130
RES, ORIGIN = 0.05, (-3.0, -2.0, 0.0)


def blank(H=H0, W=W0):
    return np.zeros((H, W), dtype=np.uint8)


def annulus(width, centre=(48.0, 64.0), mid=30.0, H=H0, W=W0):
    """free where |distance of the cell centre from `centre` - mid| < width / 2; centre in (row, column) of the IMAGE"""
    rr, cc = np.mgrid[0:H, 0:W]
    d = np.sqrt((rr + 0.5 - centre[0]) ** 2 + (cc + 0.5 - centre[1]) ** 2)
    img = blank(H, W)
    img[np.abs(d - mid) < 0.5 * width] = 255
    return img


def rect_ring(r0, r1, c0, c1, wr, wc=None, H=H0, W=W0):
    """a rectangular ring: outer box rows r0 .. r1, columns c0 .. c1 (inclusive), corridor wr cells wide in rows and wc in columns"""
    wc = wr if wc is None else wc
    img = blank(H, W)
    img[r0:r1 + 1, c0:c1 + 1] = 255
    img[r0 + wr:r1 + 1 - wr, c0 + wc:c1 + 1 - wc] = 0
    return img


ANNULI = (("annulus_w9", 9.0, (48.0, 64.0)), ("annulus_w10", 10.0, (48.5, 64.5)), ("annulus_w13", 13.0, (48.0, 64.5)))


def fixtures():
    """{name: (image, seed world point)}; every seed lies in the corridor"""
    out = {}
    for name, w, ctr in ANNULI:
        out[name] = annulus(w, ctr)
    a = annulus(10.0, (48.5, 64.5))
    s1 = a.copy()
    s1[46:51, 96:128] = 255                      # one dead-end spur of 5 x 32 cells on the outside
    out["annulus_spur"] = s1
    s3 = a.copy()
    s3[46:51, 96:128] = 255
    s3[2:16, 62:67] = 255                        # outside, upwards
    s3[45:50, 36:60] = 255                       # inside, towards the centre
    out["annulus_spurs3"] = s3
    # an inside spur that reaches the annulus' centre: where it leaves the corridor the rule keeps a four-cell diamond around an
    # empty cell, a tiny cycle that pruning cannot remove.  Refused as not a simple loop (5 of 177 cells branch).
    sd = s3.copy()
    sd[45:50, 36:60] = a[45:50, 36:60]
    sd[46:51, 40:64] = 255
    out["annulus_spur_diamond"] = sd
    bl = a.copy()
    bl[4:14, 4:14] = 255                         # a disconnected 10 x 10 blob
    out["annulus_blob"] = bl
    out["rect_w12"] = rect_ring(5, 90, 15, 114, 12)
    out["rect_w11_12"] = rect_ring(5, 90, 15, 114, 11, 12)
    out["border_ring"] = rect_ring(0, H0 - 1, 0, W0 - 1, 12)
    f8 = rect_ring(10, 85, 15, 114, 10)
    f8[10:86, 60:70] = 255                       # a bar across the middle: two loops that share it
    out["figure_eight"] = f8
    st = blank()
    st[40:52, 8:122] = 255
    out["straight"] = st
    return out


def fixture_seed(name):
    """a world point inside each fixture's corridor (table cell (48, 33 or so): on the left arm of the rings)"""
    cells = {"border_ring": (48, 6), "straight": (45, 64), "rect_w12": (48, 20), "rect_w11_12": (48, 20), "figure_eight": (48, 19)}
    r, c = cells.get(name, (47, 34))
    return cell_world(r, c)


def cell_world(r, c, res=RES, origin=ORIGIN):
    oc, os_ = np.cos(origin[2]), np.sin(origin[2])
    px, py = (c + 0.5) * res, (r + 0.5) * res
    return float(origin[0] + (px * oc - py * os_)), float(origin[1] + (px * os_ + py * oc))
