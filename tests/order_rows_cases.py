"""What the order-rows tests share (test_order_rows_names.py, test_order_rows_layouts_cpu.py, test_gpu_order_rows*.py):
the shapes, the layouts, the handles.

Shapes: N = 70 envs (not a multiple of 64), 15 zones (PointTSP-v2's config) and 5 zones, both with num_steps = 4, so an
episode ends by its time limit on the fourth step and the auto-reset falls inside a 6-frame collection.

Layouts (``set_bank``): every even env starts at the centre of its zone 0 -- the layout of a config whose robot and first
zone are pinned to the same point, keep-outs off -- so it visits that zone on its first step whatever the action (a
step moves the robot a few millimetres, a zone's radius is 0.2), and again after the auto-reset, on the fifth; every
odd env has the plain config's layout of its seed.  Routes: the built-in tour for envs 0, 1 mod 4, a fixed permutation
for the others.  test_order_rows_layouts_cpu.py checks on the CPU oracle that these layouts visit and reset as said."""
import numpy as np

N = 70
T = 6
ZONES = (15, 5)
NUM_STEPS = 4
SEED0 = 300
PIN = (0.5, -0.5)


def configs(Z, zones):
    """(the handle's config, the config whose layouts put the robot inside zone 0)."""
    base = {15: "PointTSP-v0", 5: "PointTSP-v1"}[zones]
    plain = Z.config_for_id(base, num_steps=NUM_STEPS)
    inside = Z.config_for_id(base, num_steps=NUM_STEPS, robot_locations=[PIN], zones_locations=[PIN],
                             robot_keepout=0.0, zones_keepout=0.0)
    return plain, inside


def layouts(Z, zones, n=N):
    """robots [n, 3], zone centres [n, zones, 2], ranks [n, zones] int32, seeds [n]; env i's config is
    ``configs(Z, zones)[1 - i % 2]``."""
    plain, inside = configs(Z, zones)
    rs = np.random.RandomState(zones)
    robots, zxy, ranks = [], [], []
    for i in range(n):
        robot, z, _, _ = Z.sample_layout(inside if i % 2 == 0 else plain, SEED0 + i)
        robots.append(robot)
        zxy.append(z)
        ranks.append(Z.route_ranks(robot, z) if i % 4 < 2 else rs.permutation(zones).astype(np.int32))
    return np.array(robots), np.array(zxy), np.array(ranks, np.int32), SEED0 + np.arange(n, dtype=np.int64)


def make_env(Z, zones, fresh=False, rows=True, n=N):
    """A solver-ordered handle on these layouts, reset; rows: with ``order_rows()`` on."""
    env = Z.ZoneVecEnv(configs(Z, zones)[0], n)
    env.enable_order(fresh_route_in_first_obs=fresh)
    if rows:
        env.order_rows()
    robots, zxy, ranks, seeds = layouts(Z, zones, n)
    env.set_bank(robots, zxy, aux=ranks, seeds=seeds)
    env.schedule_sequential()
    env.reset()
    return env


def want_rows(env, Z):
    """concatenate(zone_obs, order_val[..., None]) of the handle's current observation."""
    return np.concatenate([env.get(Z.F_ZONE_OBS), env.get(Z.F_ORDER_VAL)[..., None]], axis=-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gae(value, reward, mask, next_value, next_mask, discount, lam):
    """collect_experiences' recursion (main/src/torch_ac/algos/base.py:190-196) in float32, arrays [n, T]."""
    f = np.float32
    n, frames = value.shape
    adv = np.zeros((n, frames), f)
    for t in reversed(range(frames)):
        nm = mask[:, t + 1] if t + 1 < frames else next_mask
        nv = value[:, t + 1] if t + 1 < frames else next_value
        na = adv[:, t + 1] if t + 1 < frames else np.zeros(n, f)
        delta = reward[:, t] + f(discount) * nv * nm - value[:, t]
        adv[:, t] = delta + f(discount) * f(lam) * na * nm
    return adv
