"""Layouts sampled on the device (K20, layout_sample.hip) beside the unchanged host path, same box, same run.

    python scripts/layout_sample_time.py [--quick] [--slots S] [--depth D] [--only CONFIG] [--out profiles/layout_sample.json]

For PointTSP-v0, ColourMatch-v0, 25 zones at keepout 0.40 and PointTTSP-v0 (its handles switched to device-drawn
deadlines, timed_layouts_device; the host paths beside them stay the unchanged libm sampler, update_bank on a handle of
its own without the switch), S = 65 536 layouts.  --only CONFIG times one row and keeps the others of an existing --out file.  After one warm-up of every path the
paths are timed in turn, REPEATS rounds (>= 5), every timed call ending in a synchronise; the median is reported with
min .. max:

  build           build_bank_seeds(n_threads=16)        against  build_bank_seeds_device
  refill          update_bank of all S slots            against  update_bank_device, and against ring_refill with all S
                  slots stale; ring_refill with nothing stale is the fixed cost of asking
  rollout         the persistent rollout's env-steps/s at N = S envs, D steps per call (a ring of depth D allows D
                  auto-resetting steps per call), uniform policy: a sequential bank of 4096 maps walked round for ever
                  against a streamed ring with one ring_refill per call

The host figures are this box's CPU (16 threads) through the same calls a user makes.  --quick: S = 4096, 2 rounds (a
rehearsal, not a measurement)."""
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
    depth = arg("--depth", 16)
    repeats = 2 if QUICK else max(5, arg("--repeats", 5))
    calls = 4 if QUICK else 20
    out_path = arg("--out", os.path.join(ROOT, "profiles", "layout_sample.json"), str)
    configs = {"PointTSP-v0": Z.config_for_id("PointTSP-v0"), "ColourMatch-v0": Z.config_for_id("ColourMatch-v0"),
               "z25k40": Z.default_config(0, 25, zones_keepout=0.40), "PointTTSP-v0": Z.config_for_id("PointTTSP-v0")}
    result = dict(slots=S, depth=depth, repeats=repeats, host_threads=16, quick=QUICK, configs={})
    only = arg("--only", None, str)
    if only is not None:
        configs = {only: configs[only]}
        if os.path.exists(out_path):
            with open(out_path) as f:
                old = json.load(f)
            if all(old.get(k) == result[k] for k in ("slots", "depth", "quick")):
                result["configs"] = old["configs"]

    def handle(cfg, n):
        env = Z.ZoneVecEnv(cfg, n)
        if cfg.task == Z.TASK_TIMED_TSP:
            env.timed_layouts_device()
        return env
    for name, cfg in configs.items():
        row = {}
        timed_task = cfg.task == Z.TASK_TIMED_TSP
        # ---- build
        env = handle(cfg, 64)
        seeds = np.arange(1, S + 1, dtype=np.int64)
        paths = {"host": lambda: env.build_bank_seeds(seeds, n_threads=16), "device": lambda: env.build_bank_seeds_device(seeds)}
        for fn in paths.values():
            fn()
        ms = {k: [] for k in paths}
        for _ in range(repeats):
            for k, fn in paths.items():
                ms[k].append(timed(fn, env))
        row["build"] = {k: summary(v) for k, v in ms.items()}
        env.close()
        # ---- refill: one handle of S envs, a streamed ring of depth 1 = S slots
        env = handle(cfg, S)
        env.ring_stream(np.arange(S, dtype=np.int64) * 1000 + 1, 1)
        slots = np.arange(S, dtype=np.int32)
        host = env
        if timed_task:       # update_bank on a switched handle samples with the shared sampler: time the unchanged one
            host = Z.ZoneVecEnv(cfg, 64)
            host.build_bank_seeds(np.arange(1, S + 1, dtype=np.int64), n_threads=16)
        state = dict(base=10 ** 8)

        def fresh():
            state["base"] += S
            return state["base"] + np.arange(S, dtype=np.int64)
        paths = {"update_bank": lambda: (host.update_bank(slots, fresh(), n_threads=16), host.sync()),
                 "update_bank_device": lambda: env.update_bank_device(slots, fresh()),
                 "ring_refill_all_stale": env.ring_refill,          # the updates before it left no slot on its ring seed
                 "ring_refill_none_stale": env.ring_refill}
        for fn in paths.values():
            fn()
        ms = {k: [] for k in paths}
        sampled = []
        for _ in range(repeats):
            for k, fn in paths.items():
                before = env.sample_status()["n_sampled_total"]
                ms[k].append(timed(fn, env))
                st = env.sample_status()
                sampled.append((k, st["n_sampled_total"] - before, st["n_failed"]))
        row["refill"] = {k: summary(v) for k, v in ms.items()}
        row["refill_layouts_sampled_on_device"] = {k: sorted({n for kk, n, _ in sampled if kk == k}) for k in paths}
        row["refill_unfinished"] = max(f for _, _, f in sampled)
        env.close()
        if host is not env:
            host.close()
        # ---- rollout: env-steps/s of `calls` calls of `depth` steps
        rates = {"sequential_bank": [], "streamed_ring": []}
        envs = {}
        envs["sequential_bank"] = e = Z.ZoneVecEnv(cfg, S)
        e.build_bank(1, 4096, n_threads=16)
        e.schedule_sequential()
        envs["streamed_ring"] = e = handle(cfg, S)
        e.ring_stream(np.arange(S, dtype=np.int64) * 1000 + 1, depth)

        def run(k):
            e = envs[k]
            for c in range(calls):
                e.rollout(depth, Z.POLICY_UNIFORM, policy_seed=c)
                if k == "streamed_ring":
                    e.ring_refill()
        for k, e in envs.items():
            e.reset()
            run(k)
        for _ in range(repeats):
            for k, e in envs.items():
                rates[k].append(S * depth * calls / (timed(lambda: run(k), e) * 1e-3))
        row["rollout_env_steps_per_s"] = {k: dict(median=round(statistics.median(v)), min=round(min(v)), max=round(max(v)))
                                          for k, v in rates.items()}
        st = envs["streamed_ring"].sample_status()
        row["rollout_ring_layouts_sampled"] = st["n_sampled_total"] - S * depth
        row["rollout_ring_unfinished"] = st["n_failed"]
        for e in envs.values():
            e.close()
        result["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
