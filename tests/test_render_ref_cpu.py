"""tests/render_ref.py -- the numpy rasteriser the device frames are compared with -- pinned to the drawing rules of
DESIGN.md 4 "K18" by properties that do not go through the rasteriser itself: which colour the pixel holding a centre
has, how many pixels a disc covers, symmetry, the TimedTSP fade, what is skipped and what lies outside the view."""
import math

import numpy as np
import pytest

from tests import render_ref as R

RZ = R.zone_radius_of(0.2)


def _obs(x=0.0, y=0.0, dx=1.0, dy=0.0):
    return np.array([1.0, x, y, dx, dy, 0.0, 0.0, 0.0], np.float32)


def _row(x, y, rgb=(0.0, 1.0, 1.0), alpha=1.0, extra=None):
    row = [x, y, *rgb, alpha]
    if extra is not None:
        row.append(extra)
    return np.array(row, np.float32)


def _pixel_of(x, y, cfg):
    """(row, column) of the pixel that contains the point, by the rules: x = (c + 0.5) sx - view, y = view - (r + 0.5) sy."""
    sx, sy = 2.0 * cfg["view"] / cfg["width"], 2.0 * cfg["view"] / cfg["height"]
    return int(math.floor((cfg["view"] - y) / sy)), int(math.floor((x + cfg["view"]) / sx))


FAR = _obs(x=50.0, y=50.0)          # a robot far outside every view used here


@pytest.mark.parametrize("cfg", [dict(R.DEFAULT_CFG), dict(width=64, height=48, view=1.0, robot_radius=0.1),
                                 dict(width=31, height=129, view=2.0, robot_radius=0.3)])
def test_the_pixel_holding_a_zone_centre_has_its_colour(cfg):
    zones = np.stack([_row(-0.6, 0.4, (0.0, 1.0, 1.0)), _row(0.3, -0.7, (1.0, 1.0, 0.0)), _row(0.8, 0.8, (0.0, 0.0, 1.0))])
    img = R.render_ref(FAR, zones, 0, RZ, cfg=cfg)
    for row, want in zip(zones, [(0, 255, 255), (255, 255, 0), (0, 0, 255)]):
        r, c = _pixel_of(float(row[0]), float(row[1]), cfg)
        assert tuple(img[r, c]) == want
    assert tuple(img[0, 0]) == R.BACKGROUND and img.shape == (cfg["height"], cfg["width"], 3) and img.dtype == np.uint8


def test_painters_order_later_zone_overwrites_earlier():
    zones = np.stack([_row(0.0, 0.0, (0.0, 1.0, 1.0)), _row(0.0, 0.0, (1.0, 1.0, 0.0))])
    r, c = _pixel_of(0.001, 0.001, R.DEFAULT_CFG)
    assert tuple(R.render_ref(FAR, zones, 0, RZ)[r, c]) == (255, 255, 0)
    assert tuple(R.render_ref(FAR, zones[::-1], 0, RZ)[r, c]) == (0, 255, 255)
    # the robot is drawn over a zone, the mark between them
    img = R.render_ref(_obs(0.0, 0.0), zones, 0, RZ, mark=(0.0, 0.0))
    assert tuple(img[r, c]) in (R.BODY, R.NOSE)


@pytest.mark.parametrize("angle", [0.0, 0.7, math.pi / 2, 2.5, -2.0])
def test_the_robot_centre_pixel_is_body_and_the_pixel_ahead_is_nose(angle):
    cfg = dict(width=200, height=200, view=1.25, robot_radius=0.3)
    dx, dy = math.cos(angle), math.sin(angle)
    x0, y0 = 0.31, -0.22
    img = R.render_ref(_obs(x0, y0, dx, dy), np.zeros((0, 6), np.float32), 0, RZ, cfg=cfg)
    rad = 0.3 / 3.0
    assert tuple(img[_pixel_of(x0, y0, cfg)]) == R.BODY               # dot = ~0 <= 0.4 rad
    assert tuple(img[_pixel_of(x0 + 0.8 * rad * dx, y0 + 0.8 * rad * dy, cfg)]) == R.NOSE
    assert tuple(img[_pixel_of(x0 - 0.8 * rad * dx, y0 - 0.8 * rad * dy, cfg)]) == R.BODY
    assert tuple(img[_pixel_of(x0 + 1.3 * rad * dx, y0 + 1.3 * rad * dy, cfg)]) == R.BACKGROUND
    # a robot without a heading (the idle env's all-zero observation) has no nose
    img = R.render_ref(_obs(x0, y0, 0.0, 0.0), np.zeros((0, 6), np.float32), 0, RZ, cfg=cfg)
    colours = {tuple(p) for p in img.reshape(-1, 3)}
    assert colours == {R.BACKGROUND, R.BODY}


@pytest.mark.parametrize("cfg,rad_world", [(dict(width=100, height=100, view=1.25, robot_radius=0.1), None),
                                           (dict(width=64, height=200, view=1.0, robot_radius=0.9), 0.9),
                                           (dict(width=333, height=77, view=0.5, robot_radius=0.45), 0.45)])
def test_disc_pixel_counts(cfg, rad_world):
    """pi rad^2 / (sx sy) +- (2 pi rad / min(sx, sy) + 4): the area in pixels, give or take the pixels on the rim."""
    sx, sy = 2.0 * cfg["view"] / cfg["width"], 2.0 * cfg["view"] / cfg["height"]

    def check(count, rad):
        assert abs(count - math.pi * rad * rad / (sx * sy)) <= 2 * math.pi * rad / min(sx, sy) + 4, (count, rad)
    if rad_world is None:           # a zone disc and the mark's ring around another point
        img = R.render_ref(FAR, _row(0.1, -0.05)[None], 0, RZ, cfg=cfg)
        check(int((img == (0, 255, 255)).all(-1).sum()), float(RZ))
        img = R.render_ref(FAR, np.zeros((0, 6), np.float32), 0, RZ, mark=(0.2, 0.3), cfg=cfg)
        ring = int((img == R.MARK).all(-1).sum())
        outer, inner = 1.35 * float(RZ), float(RZ)
        area = math.pi * (outer * outer - inner * inner) / (sx * sy)
        assert abs(ring - area) <= 2 * math.pi * (outer + inner) / min(sx, sy) + 8
    else:
        img = R.render_ref(_obs(0.03, 0.02), np.zeros((0, 6), np.float32), 0, RZ, cfg=cfg)
        check(int((img != R.BACKGROUND).any(-1).sum()), rad_world / 3.0)


def test_a_mirrored_scene_gives_the_mirrored_image():
    """64 x 64 at view 1.25: the pixel pitch 2.5 / 64 and every centre are exact in float32, so the columns are
    symmetric to the bit and so is every distance."""
    cfg = dict(width=64, height=64, view=1.25, robot_radius=0.25)
    rs = np.random.RandomState(5)
    zones = np.stack([_row(*rs.uniform(-1, 1, 2), rgb=rs.randint(0, 2, 3).astype(float)) for _ in range(9)])
    obs = _obs(0.4, -0.3, math.cos(0.9), math.sin(0.9))
    mark = (0.55, 0.65)
    img = R.render_ref(obs, zones, 0, RZ, mark=mark, cfg=cfg)
    for sgn_x, sgn_y, flip in ((-1, 1, lambda a: a[:, ::-1]), (1, -1, lambda a: a[::-1]), (-1, -1, lambda a: a[::-1, ::-1])):
        z2 = zones.copy()
        z2[:, 0] *= sgn_x
        z2[:, 1] *= sgn_y
        o2 = obs.copy()
        o2[[1, 3]] *= sgn_x
        o2[[2, 4]] *= sgn_y
        got = R.render_ref(o2, z2, 0, RZ, mark=(sgn_x * mark[0], sgn_y * mark[1]), cfg=cfg)
        assert np.array_equal(got, flip(img))
    assert len({tuple(p) for p in img.reshape(-1, 3)}) >= 5


@pytest.mark.parametrize("t,want", [(1.0, (0, 255, 255)), (0.5, (128, 128, 128)), (0.0, (255, 0, 0)), (-0.1, (255, 0, 0))])
def test_timed_tsp_fade(t, want):
    row = _row(0.0, 0.0, (0.0, 1.0, 1.0), extra=t)
    assert tuple(int(v) for v in R.zone_colour(row, R.TASK_TIMED_TSP)) == want
    img = R.render_ref(FAR, row[None], R.TASK_TIMED_TSP, RZ)
    assert tuple(img[_pixel_of(0.001, 0.001, R.DEFAULT_CFG)]) == want
    # only the unvisited colour fades, and only in TimedTSP
    visited = _row(0.0, 0.0, (1.0, 1.0, 0.0), extra=t)
    assert tuple(int(v) for v in R.zone_colour(visited, R.TASK_TIMED_TSP)) == (255, 255, 0)
    assert tuple(int(v) for v in R.zone_colour(row, 0)) == (0, 255, 255)


def test_colour_conversion_clamps_and_rounds():
    assert [int(R.to_byte(c)) for c in (-3.0, 0.0, 0.001, 0.0019, 0.002, 0.5, 0.998, 1.0, 7.0)] == \
        [0, 0, 0, 0, 1, 128, 254, 255, 255]


def test_alpha_zero_rows_and_objects_outside_the_view_change_nothing():
    empty = R.render_ref(FAR, np.zeros((0, 6), np.float32), 0, RZ)
    assert (empty == R.BACKGROUND).all()
    skipped = np.stack([_row(0.0, 0.0, alpha=0.0), np.zeros(6, np.float32)])
    assert np.array_equal(R.render_ref(FAR, skipped, 0, RZ), empty)
    outside = np.stack([_row(1.25 + 0.07, 0.0), _row(0.0, -1.4), _row(-3.0, 3.0)])     # radius 0.0667: wholly outside
    assert np.array_equal(R.render_ref(_obs(1.3, 1.3), outside, 0, RZ, mark=(5.0, 5.0)), empty)
    assert np.array_equal(R.render_ref(FAR, outside[:0], 0, RZ, mark=(np.nan, 0.0)), empty)
    assert np.array_equal(R.render_ref(FAR, outside[:0], 0, RZ, mark=(0.0, np.nan)), empty)
    touching = R.render_ref(FAR, _row(1.25 + 0.05, 0.0)[None], 0, RZ)                   # reaches 0.017 into the view
    assert not np.array_equal(touching, empty)
