"""Layouts for the route solver's tests (tests/test_route_solver_shared.py, tests/test_gpu_route_solver.py): sampled
ones, and crafted ones where arcs tie, vanish or exceed 2^31."""
import numpy as np

CRAFTED_Z = (3, 4, 15, 31, 32)


def crafted(Z):
    """[(name, robot (2,), zones (Z, 2))] -- every layout twice where the order of the zones matters: as built and
    under a fixed permutation (ties are broken by index)."""
    rng = np.random.default_rng(1000 + Z)
    perm = rng.permutation(Z)
    k = np.arange(Z, dtype=np.float64)
    out = []

    def add(name, robot, zones, permuted=True):
        zones = np.ascontiguousarray(zones, np.float64).reshape(Z, 2)
        robot = np.asarray(robot, np.float64)
        out.append((name, robot, zones))
        if permuted:
            out.append((name + "-permuted", robot, np.ascontiguousarray(zones[perm])))

    # equally spaced collinear zones: from one end, and with the robot in the middle
    line = np.stack([0.3 * (k + 1), np.zeros(Z)], 1)
    add("collinear", (0.0, 0.0), line)
    add("collinear-middle", (0.3 * (Z // 2) + 0.15, 0.0), line)
    # a circle centred on the robot: every depot arc ties (up to the square root's rounding)
    ang = 2 * np.pi * k / Z
    add("circle", (0.5, -0.25), np.stack([0.5 + np.cos(ang), -0.25 + np.sin(ang)], 1))
    # integer grid points: ties everywhere after truncation
    w = int(np.ceil(np.sqrt(Z + 1)))
    add("grid", (0.0, 0.0), np.stack([(k + 1) % w, (k + 1) // w], 1))
    add("grid-tenths", (0.0, 0.0), 0.1 * np.stack([(k + 1) % w, (k + 1) // w], 1))
    # repeated points and all-equal points: zero arcs
    pts = rng.uniform(-2, 2, (max(1, Z // 3), 2))
    add("repeated", (0.1, 0.2), pts[np.arange(Z) % len(pts)])
    add("all-equal", (0.0, 0.0), np.tile([[1.0, 1.0]], (Z, 1)), permuted=False)
    add("all-on-the-robot", (1.0, 1.0), np.tile([[1.0, 1.0]], (Z, 1)), permuted=False)
    # coordinates near 1e8: costs beyond 2^31 pin the int64 semantics
    big = rng.uniform(-1.0, 1.0, (Z + 1, 2)) * 1e8
    big[0], big[1] = (-1e8, -1e8), (1e8, 1e8)             # this arc alone costs 2.83e9
    add("1e8", big[0], big[1:])
    add("1e8-grid", (0.0, 0.0), 1.9e8 * np.stack([(k + 1) % w, (k + 1) // w], 1))     # its diagonals cost 2.69e9
    return out


def sampled(Z, cfg, seeds):
    """(robot (n, 2), zones (n, Z, 2)) of the host sampler's layouts."""
    rows = [Z.sample_layout(cfg, int(s)) for s in seeds]
    return (np.ascontiguousarray([r[0][:2] for r in rows], np.float64),
            np.ascontiguousarray([r[1] for r in rows], np.float64))
