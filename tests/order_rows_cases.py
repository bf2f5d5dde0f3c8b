"""What the order-rows tests share (test_order_rows_names.py, test_order_rows_layouts_cpu.py, test_gpu_order_rows*.py):
the shapes, the layouts, the handles.

Shapes: N = 70 envs (not a multiple of 64), 15 zones (PointTSP-v2's config) and 5 zones, both with num_steps = 4, so an
episode ends by its time limit on the fourth step and the auto-reset falls inside a 6-frame collection.

Layouts (``set_bank``): every even env starts at the centre of its zone 0 -- the layout of a config whose robot and first
zone are pinned to the same point, keep-outs off -- so it visits that zone on its first step whatever the action (a
step moves the robot a few millimetres, a zone's radius is 0.2), and again after the auto-reset, on the fifth; every
odd env has the plain config's layout of its seed.  Routes: the built-in tour for envs 0, 1 mod 4, a fixed permutation
for the others.  test_order_rows_layouts_cpu.py checks on the CPU oracle that these layouts visit and reset as said.

Edge shapes (CASES, for test_gpu_order_edges.py): the same layouts and routes at batch sizes and zone counts that move
K22's 16-byte store grid, K7's 256-thread launch edge and the zone loop's ends; ``lead_tail`` says which pieces K22
writes for frame slot t of a collection.  Zone counts without a registry id come from ``default_config(0, zones)``, with
zones_keepout = 0.30 at 32 zones (the default keep-out leaves no room for 32)."""
import numpy as np

N = 70
T = 6
ZONES = (15, 5)
NUM_STEPS = 4
SEED0 = 300
PIN = (0.5, -0.5)
BASE_IDS = {15: "PointTSP-v0", 5: "PointTSP-v1"}

# name: (envs, zones).  7 * N * Z mod 4 decides which (lead, tail) pairs K22 runs on the slots of a collection:
#   one      3  the smallest launch, 7 floats: leads 0, 1, 2, 3 on frames 0..3, lead 3 leaves exactly one whole piece
#   odd15    1  leads 0, 3, 2, 1 and tails 1, 2, 3, 0; N * T * Z * 7 is odd for odd T (exp.action at an odd float offset)
#   blocks3  3  569 pieces: three workgroups, with odd leads
#   edge257  1  past K7's 256-thread launch edge, many workgroups of K22, the compile-time Z = 15
#   edge256  0  fully aligned control, Z = 2
#   edge255  1  just below the launch edge
#   z32      0  the largest zone count: the feature reaches 2^-31, int8 positions reach 31
#   base15, base5   2  the N = 70 shapes of the older tests
CASES = {"one": (1, 1), "odd15": (3, 5), "blocks3": (65, 5), "edge257": (257, 15), "edge256": (256, 2),
         "edge255": (255, 5), "z32": (2, 32), "base15": (N, 15), "base5": (N, 5)}
EDGE_CASES = ("one", "odd15", "blocks3", "edge257", "edge256", "edge255", "z32")


def lead_tail(n, zones, t):
    """What K22 writes around its 16-byte store grid for frame slot t of a collection on n envs: slot t starts
    t * total floats (total = 7 * n * zones) behind a 16-byte-aligned base, so ``lead`` floats come before the first
    aligned one and the last piece is cut to ``tail`` floats (0: the grid ends with the slot)."""
    total = 7 * n * zones
    lead = (-t * total) % 4
    return lead, (total - lead) % 4


def configs(Z, zones, num_steps=NUM_STEPS, **over):
    """(the handle's config, the config whose layouts put the robot inside zone 0)."""
    inside = dict(robot_locations=[PIN], zones_locations=[PIN], robot_keepout=0.0, zones_keepout=0.0)
    if zones in BASE_IDS:
        return (Z.config_for_id(BASE_IDS[zones], num_steps=num_steps, **over),
                Z.config_for_id(BASE_IDS[zones], num_steps=num_steps, **dict(over, **inside)))
    keepout = {"zones_keepout": 0.30} if zones == 32 else {}
    return (Z.default_config(0, zones, num_steps=num_steps, **dict(keepout, **over)),
            Z.default_config(0, zones, num_steps=num_steps, **dict(over, **inside)))


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


def make_env(Z, zones, fresh=False, rows=True, n=N, num_steps=NUM_STEPS, **over):
    """A solver-ordered handle on these layouts, reset; rows: with ``order_rows()`` on; over: config overrides of the
    handle (``kernel``)."""
    env = Z.ZoneVecEnv(configs(Z, zones, num_steps, **over)[0], n)
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
