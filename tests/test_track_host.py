"""CPU-only: f1tenth_gym_amd.Track (track progress) — validation, segment lengths, cum and L, the ds wrap rule, and
the NumPy restatement of the projection against the oracle's nearest_on_trajectory (the reference's
nearest_point_on_trajectory, examples/waypoint_follow.py:15-50)."""
import os

import numpy as np
import pytest

from _util import MAPS, raceline


def _wp3(xy):
    """the [M][3] waypoint layout the oracle reads (x, y, speed)"""
    return np.column_stack([xy, np.zeros(len(xy))])


@pytest.mark.parametrize("xy, closed, what", [
    ([[0.0, 0.0]], False, "at least 2 points"),
    ([[0.0, 0.0], [1.0, 0.0]], True, "at least 3 distinct"),
    ([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]], True, "at least 3 distinct"),     # the repeat is dropped first
    ([[0.0, 0.0], [np.nan, 0.0], [1.0, 1.0]], False, "finite"),
    ([[0.0, 0.0], [np.inf, 0.0], [1.0, 1.0]], True, "finite"),
    ([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [2.0, 0.0]], False, "zero length"),
    ([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 1.0]], True, "zero length"),
    ([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0]], False, "[M][2]"),
])
def test_track_refusals(xy, closed, what):
    from f1tenth_gym_amd import Track
    with pytest.raises(ValueError) as ei:
        Track.from_xy(np.array(xy), closed=closed)
    assert what in str(ei.value)


def test_closing_repeat_is_dropped_only_when_bitwise_equal():
    from f1tenth_gym_amd import Track
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    t = Track.from_xy(np.vstack([sq, sq[:1]]))
    assert t.num_points == 4 and t.num_segments == 4 and t.length == 4.0
    near = np.vstack([sq, [[0.0, 1e-9]]])          # not bitwise the first point: kept, closing segment 1e-9 long
    assert Track.from_xy(near).num_points == 5
    t_open = Track.from_xy(np.vstack([sq, sq[:1]]), closed=False)   # open: nothing dropped, the loop's 4 segments
    assert t_open.num_points == 5 and t_open.num_segments == 4 and t_open.length == 4.0


def test_cum_and_length_open_and_closed():
    from f1tenth_gym_amd import Track
    xy = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 10.0], [-1.0, 10.0]])
    o = Track.from_xy(xy, closed=False)
    assert o.num_segments == 3
    np.testing.assert_array_equal(o.seg_len, [5.0, 6.0, 4.0])
    np.testing.assert_array_equal(o.cum, [0.0, 5.0, 11.0])
    assert o.length == 15.0
    c = Track.from_xy(xy, closed=True)
    assert c.num_segments == 4
    np.testing.assert_array_equal(c.seg_len[:3], [5.0, 6.0, 4.0])
    assert c.seg_len[3] == np.sqrt(1.0 + 100.0)
    np.testing.assert_array_equal(c.cum, [0.0, 5.0, 11.0, 15.0])
    assert c.length == 15.0 + np.sqrt(101.0)
    # the running float64 sum, in order
    rng = np.random.default_rng(3)
    pts = np.cumsum(rng.uniform(0.1, 1.0, (500, 2)), axis=0)
    t = Track.from_xy(pts, closed=False)
    acc, want = 0.0, []
    for v in np.sqrt(np.sum(np.diff(pts, axis=0) ** 2, axis=1)):
        want.append(acc)
        acc += v
    np.testing.assert_array_equal(t.cum, want)
    assert t.length == acc


def test_example_raceline_length_and_segments():
    """the shipped csv (x, y in columns 1, 2): its last row repeats row 0 and is dropped; closed, 782 points make 782 segments"""
    from f1tenth_gym_amd import Track
    path = os.path.join(MAPS, "example_waypoints.csv")
    t = Track.from_csv(path, xind=1, yind=2, delim=';', skiprows=3)
    w = raceline()
    assert w.shape[0] == 783 and np.array_equal(w[-1, 1:3], w[0, 1:3])
    assert t.num_points == 782 and t.num_segments == 782 and t.closed
    assert round(t.length, 5) == 156.35612
    # the same as the open polyline of all 783 rows
    assert Track.from_xy(w[:, 1:3], closed=False).length == t.length
    assert Track.coerce(path).length == t.length


def test_ds_wrap_rule():
    from f1tenth_gym_amd import Track
    t = Track.from_xy([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])   # L = 16
    L = t.length
    got = t.wrap_ds([0.0, 8.0, -8.0, 8.0 + 1e-9, -8.0 + 1e-9, 15.0, -15.0, 7.5])
    np.testing.assert_array_equal(got, [0.0, 8.0, 8.0, 8.0 + 1e-9 - L, -8.0 + 1e-9, -1.0, 1.0, 7.5])
    o = Track.from_xy([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0]], closed=False)
    np.testing.assert_array_equal(o.wrap_ds([7.0, -7.0]), [7.0, -7.0])


def _check_against_oracle(track, poses):
    from oracle import orc
    got = track.project(poses)
    wp = _wp3(track.points_closed())
    for r, (px, py, th) in enumerate(poses):
        i, dist, t = orc.nearest_on_trajectory(wp, px, py)
        assert got[r, 3] == i and got[r, 4] == t, (r, got[r], i, t)
        assert abs(got[r, 1]) == dist
        assert got[r, 0] == track.cum[i] + t * track.seg_len[i]


def test_numpy_projection_equals_oracle():
    from f1tenth_gym_amd import Track
    w = raceline()
    rl = Track.from_xy(w[:, 1:3])
    rng = np.random.default_rng(11)
    lo, hi = w[:, 1:3].min(axis=0) - 3.0, w[:, 1:3].max(axis=0) + 3.0
    poses = np.column_stack([rng.uniform(lo[0], hi[0], 2000), rng.uniform(lo[1], hi[1], 2000), rng.uniform(-7, 7, 2000)])
    poses[:200, :2] = w[rng.integers(0, 782, 200), 1:3]      # on vertices
    _check_against_oracle(rl, poses)
    # an open and a closed small track, points equidistant from two segments (the first index wins)
    sq = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]])
    eq = np.array([[1.0, 1.0, 0.0], [1.0, 0.5, 1.0], [0.5, 1.0, -1.0], [3.0, 3.0, 0.0], [-1.0, -1.0, 2.0], [1.0, -5.0, 0.0]])
    for closed in (True, False):
        t = Track.from_xy(sq, closed=closed)
        _check_against_oracle(t, eq)
        _check_against_oracle(t, np.column_stack([rng.uniform(-3, 5, (1000, 2)), rng.uniform(-4, 4, 1000)]))
    assert Track.from_xy(sq).project(eq[:1])[0, 3] == 0      # (1, 1): distance 1 from all four sides -> segment 0


def test_lateral_sign_and_heading_error():
    from f1tenth_gym_amd import Track
    t = Track.from_xy([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])
    out = t.project([[5.0, 1.0, 0.25], [5.0, -1.0, -0.25], [5.0, 0.5, np.pi], [5.0, 0.5, -np.pi]])
    np.testing.assert_array_equal(out[:, 0], [5.0, 5.0, 5.0, 5.0])
    np.testing.assert_array_equal(out[:, 1], [1.0, -1.0, 0.5, 0.5])     # left of +x is +y
    np.testing.assert_allclose(out[:, 2], [0.25, -0.25, -np.pi, -np.pi])   # [-pi, pi)
    assert np.all(out[:, 2] >= -np.pi) and np.all(out[:, 2] < np.pi)
