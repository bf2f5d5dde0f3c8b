"""The solver-ordered handles' tour on the device (K21, layout_sample.hip) beside the host path, same box, same run.

    python scripts/route_solve_time.py [--quick] [--slots S] [--only CONFIG] [--out profiles/route_solve.json]

For PointTSP-v0 (15 zones) and 25 zones at keepout 0.40, S = 65 536 layouts.  After one warm-up of every path the paths
are timed in turn, REPEATS rounds (>= 5), every timed call ending in a synchronise; the median is reported with
min .. max:

  host_order_build      build_bank_seeds(n_threads=16) on a solver-ordered handle: the host sampler, then route_ranks per
                        layout, then the upload -- the path a solver-ordered env had before K21
  device_order_build    build_bank_seeds_device on a solver-ordered handle with order_routes_device() on: the wave that
                        samples a layout solves its tour
  device_plain_build    build_bank_seeds_device on a plain handle of the same config; device_order_build minus this is
                        the solver's share
  route_ranks_device    the batch kernel alone over the same S layouts (host arrays in, host arrays out: the copies are
                        in the figure)

The host figures are this box's CPU (16 threads) through the same calls a user makes.  The banks of the two solver-ordered
builds are compared once, bit for bit.  --quick: S = 4096, 2 rounds (a rehearsal, not a measurement)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, env):
    env.sync()
    t0 = time.perf_counter()
    fn()
    env.sync()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def main():
    sys.path.insert(0, ROOT)
    import combinatorial_rl_tasks_amd as Z

    S = arg("--slots", 4096 if QUICK else 65536)
    repeats = 2 if QUICK else max(5, arg("--repeats", 5))
    out_path = arg("--out", os.path.join(ROOT, "profiles", "route_solve.json"), str)
    configs = {"PointTSP-v0": Z.config_for_id("PointTSP-v0"), "z25k40": Z.default_config(0, 25, zones_keepout=0.40)}
    only = arg("--only", None, str)
    if only is not None:
        configs = {only: configs[only]}
    result = dict(slots=S, repeats=repeats, host_threads=16, quick=QUICK, configs={})
    seeds = np.arange(1, S + 1, dtype=np.int64)
    for name, cfg in configs.items():
        order_host, order_dev, plain = (Z.ZoneVecEnv(cfg, 64) for _ in range(3))
        for env in (order_host, order_dev):
            env.enable_order()
        order_dev.order_routes_device()
        # the layouts the batch kernel is timed on: the bank's own
        plain.build_bank_seeds_device(seeds)
        bank = plain.read_bank()
        robot = np.ascontiguousarray(bank["robot"][:, :2])
        zones = bank["zone_xy"]
        paths = {"host_order_build": (order_host, lambda: order_host.build_bank_seeds(seeds, n_threads=16)),
                 "device_order_build": (order_dev, lambda: order_dev.build_bank_seeds_device(seeds)),
                 "device_plain_build": (plain, lambda: plain.build_bank_seeds_device(seeds)),
                 "route_ranks_device": (plain, lambda: plain.route_ranks_device(robot, zones))}
        for env, fn in paths.values():
            fn()
        a, b = order_host.read_bank(), order_dev.read_bank()
        same = all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in a)
        ranks, moves = plain.route_ranks_device(robot, zones, moves=True)
        same = same and np.array_equal(ranks, a["aux"])
        ms = {k: [] for k in paths}
        for _ in range(repeats):
            for k, (env, fn) in paths.items():
                ms[k].append(timed(fn, env))
        row = {k: summary(v) for k, v in ms.items()}
        row["solver_share_ms"] = round(row["device_order_build"]["median_ms"] - row["device_plain_build"]["median_ms"], 4)
        row["host_over_device"] = round(row["host_order_build"]["median_ms"] / row["device_order_build"]["median_ms"], 2)
        row["banks_equal"] = bool(same)
        row["moves_per_layout"] = dict(mean=round(float(moves.sum(1).mean()), 3), max=int(moves.sum(1).max()),
                                       per_operator_mean=[round(float(x), 4) for x in moves.mean(0)])
        row["unfinished"] = order_dev.sample_status()["n_failed"]
        for env in (order_host, order_dev, plain):
            env.close()
        result["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
