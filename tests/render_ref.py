"""A numpy float32 rasteriser written from the drawing rules of DESIGN.md 4 "K18" (include/zenv.h, zenv_render): the
reference the device frames are compared with, byte for byte.  Every operation is a float32 numpy operation in the
order the rules give -- one rounding per product, sum and difference, as the kernel's contraction-free float32 -- so
there is no tolerance anywhere.

    render_ref(obs [8], zone_obs [Z, F], task, zone_radius, mark=None, cfg=None) -> uint8 [H, W, 3]

cfg: dict(width, height, view, robot_radius), DEFAULT_CFG's values for the keys it leaves out.
"""
import numpy as np

TASK_TIMED_TSP = 1
BACKGROUND = (224, 224, 224)
MARK = (255, 0, 255)
BODY = (32, 32, 32)
NOSE = (255, 255, 255)
DEFAULT_CFG = dict(width=100, height=100, view=1.25, robot_radius=0.1)

f32 = np.float32


def zone_radius_of(zones_size):
    """(float)(cfg.zones_size / 3.0): the double quotient, then rounded to float32."""
    return f32(float(zones_size) / 3.0)


def to_byte(c):
    """A colour component: clamped to [0, 1] (a NaN becomes 0), then (uint8)floorf(c * 255 + 0.5)."""
    c = np.fmin(np.fmax(f32(c), f32(0.0)), f32(1.0))
    return np.uint8(np.floor(c * f32(255.0) + f32(0.5)))


def zone_colour(row, task):
    """RGB bytes of a zone row; an unvisited TimedTSP zone (0, 1, 1) fades with t = row[6] (TTSP_env.py:52-58)."""
    r, g, b = f32(row[2]), f32(row[3]), f32(row[4])
    if task == TASK_TIMED_TSP and r == 0.0 and g == 1.0 and b == 1.0:
        t = f32(row[6])
        r = f32(1.0) - t
        g = b = np.fmax(f32(0.0), t)
    return (to_byte(r), to_byte(g), to_byte(b))


def pixel_centres(width, height, view):
    """x [W] and y [H] of the pixel centres, observation units; row 0 is the top (+y)."""
    view = f32(view)
    sx = (f32(2.0) * view) / f32(width)
    sy = (f32(2.0) * view) / f32(height)
    x = (np.arange(width, dtype=f32) + f32(0.5)) * sx - view
    y = view - (np.arange(height, dtype=f32) + f32(0.5)) * sy
    return x, y, sx, sy


def _dist2(x, y, cx, cy):
    dx = x[None, :] - f32(cx)
    dy = y[:, None] - f32(cy)
    return dx, dy, dx * dx + dy * dy


def render_ref(obs, zone_obs, task, zone_radius, mark=None, cfg=None):
    c = dict(DEFAULT_CFG)
    c.update(cfg or {})
    W, H = int(c["width"]), int(c["height"])
    obs = np.asarray(obs, f32)
    zone_obs = np.asarray(zone_obs, f32)
    x, y, _, _ = pixel_centres(W, H, c["view"])
    img = np.empty((H, W, 3), np.uint8)
    img[...] = BACKGROUND
    rz = f32(zone_radius)
    rz2 = rz * rz
    with np.errstate(invalid="ignore"):
        for row in zone_obs:                                        # painter's order: zone 0 first
            if row[5] == 0.0:                                       # alpha 0: WaitWrapper's all-zero observation
                continue
            _, _, d2 = _dist2(x, y, row[0], row[1])
            img[d2 <= rz2] = zone_colour(row, task)
        if mark is not None and not (np.isnan(mark[0]) or np.isnan(mark[1])):
            outer = f32(1.35) * rz
            _, _, d2 = _dist2(x, y, mark[0], mark[1])
            img[(rz2 < d2) & (d2 <= outer * outer)] = MARK
        rr = f32(c["robot_radius"]) / f32(3.0)
        dx, dy, d2 = _dist2(x, y, obs[1], obs[2])
        inside = d2 <= rr * rr
        ahead = dx * obs[3] + dy * obs[4] > f32(0.4) * rr
        img[inside & ~ahead] = BODY
        img[inside & ahead] = NOSE
    return img
